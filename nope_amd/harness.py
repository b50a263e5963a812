"""Evaluation harness -- counterpart of the reference's `test_shapeNet.py`, which the README
names (README.md:82) but the tree does not contain.

Builds the model from the values of configs/model/template_base.yaml, feeds batches shaped
like `ShapeNet.__getitem__` on the test split (src/dataloader/shapeNet.py:348-357, keyed
"shapeNet_<category>" as model.py:551-552 expects) and runs the hot path:
`generate_templates -> retrieval -> template_poses[0][nearest_idx]` (model.py:313,323,352),
then the geodesic angle / Acc@{15,30} (loss.py:76-115; non-symmetric branch only).  There is
no dataset and no checkpoint in the tree or on the box, so images, poses and weights are
synthetic and seeded; the numbers are plumbing checks, not accuracy claims.  It does not
replicate the reference's `vis_imgs` UnboundLocalError (model.py:367): without visualisation
predictions are saved with `query_pose` and `similarity` only; with it (`--visualize`, the VAE
encoder and `--save-dir`) the pictures, the video and `vis_imgs` are written (nope_amd/vis.py).

    python -m nope_amd.harness --batch 1 --templates 64 --size 128     # BASELINE config 1 shape

With a dataset on disk (`--data-root`, the reference's rendered ShapeNet layout) the same loop runs over a testing split read by
`nope_amd.dataset.ShapeNet`: load_batch -> eval_geodesic per batch, then ONE JSON line with the split's sample-weighted Acc@15 / Acc@30 and
the median over all samples' errors.  Weights stay synthetic unless a checkpoint is loaded by the caller.

    python -m nope_amd.harness --data-root DIR --split bottle --id2cat FILE [--fast] [--limit N] [--batch B] [--visualize --save-dir DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import Dict, Optional

import numpy as np
import torch

from . import hip

TEMPLATE_BASE = dict(          # configs/model/template_base.yaml
    u_net=dict(u_net_dim=192, rot_representation_dim=6, pose_mlp_name="single_layer",
               encoder=dict(descriptor_size=8, threshold=0.2, normalize=False)),
    optim_config=dict(loss_type="l1", lr=5e-5, weight_decay=0.0005, warm_up_steps=500, use_inv_deltaR=True),
    testing_config=dict(similarity_metric="l2"),
)


class StubEncoder(torch.nn.Module):
    """An encoder that hands embeddings through unchanged: exactly what UNet / PoseConditional read from an encoder (`latent_dim`, `name`,
    `encode_image`, u_net.py:44-46, model.py:107-108) and nothing else.  Scoring-only runs and operator-level checks build a U-Net
    around it when the images are already embeddings."""

    def __init__(self, latent_dim=8):
        super().__init__()
        self.latent_dim = latent_dim
        self.name = "template"

    @torch.no_grad()
    def encode_image(self, image, mode=None):
        return image


def random_rotations(n: int, gen: torch.Generator) -> torch.Tensor:
    """Haar-distributed rotations, float64 (n,3,3): QR of a Gaussian with sign fix."""
    a = torch.randn(n, 3, 3, generator=gen, dtype=torch.float64)
    q, r = torch.linalg.qr(a)
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1)).unsqueeze(-2)
    det = torch.linalg.det(q)
    q[:, :, 0] = q[:, :, 0] * det.unsqueeze(-1)
    return q


def rotation_6d(m: torch.Tensor) -> torch.Tensor:
    """6D representation = first two rows, flattened (src/poses/rotation_conversions.py:490-503)."""
    return m[..., :2, :].clone().reshape(*m.shape[:-2], 6)


def synthetic_batch(batch: int, n_templates: int, size: int, seed: int = 2022, device="cpu",
                    pose_level: Optional[int] = None, pose_root: Optional[str] = None, gt_templates: bool = False,
                    n_references: int = 1) -> Dict[str, torch.Tensor]:
    """A test-split batch shaped like ShapeNet.__getitem__ (dataloader/shapeNet.py:348-357).  Template poses are
    Haar-random rotations, or -- `pose_level` 0..3 -- the upper-hemisphere icosphere grid the reference evaluates on
    (nope_amd.poses: 26 / 91 / 341 / 1321 viewpoints; `pose_root` = the reference's predefined_poses directory to
    read its own files); `n_templates` is ignored then.  gt_templates: add the (B, N, 3, size, size) ground-truth template images that the
    visualisation shows (shapeNet.py:352; drawn last, the other tensors do not change).  n_references R (no reference counterpart: the
    reference's test split has one reference per object): `references` (B, R, 3, size, size) and `reference_poses` (B, R, 3, 3) for the
    multi-reference path; index 0 is `reference` and its pose, the extras are drawn after everything else."""
    g = torch.Generator().manual_seed(seed)
    query = torch.rand(batch, 3, size, size, generator=g) * 2 - 1
    reference = torch.rand(batch, 3, size, size, generator=g) * 2 - 1
    if pose_level is not None:
        from .poses import get_obj_poses_from_template_level
        grid = get_obj_poses_from_template_level(pose_level, "upper", root=pose_root)
        R_tpl = torch.from_numpy(grid[:, :3, :3].copy())
        n_templates = R_tpl.shape[0]
    else:
        R_tpl = random_rotations(n_templates, g)
    R_ref = random_rotations(batch, g)
    R_query = random_rotations(batch, g)
    rel = lambda a, b: a @ torch.linalg.inv(b)          # shapeNet.py:243-245
    all_rel = rotation_6d(rel(R_tpl[None], R_ref[:, None])).float()
    gt_rel = rotation_6d(rel(R_query, R_ref)).float()
    out = dict(query=query, reference=reference, gt_relativeR=gt_rel, all_relativeR=all_rel,
               symmetry=torch.zeros(batch, 1), query_pose=R_query,
               template_poses=R_tpl[None].expand(batch, -1, -1, -1).contiguous())
    if gt_templates:
        out["gt_templates"] = torch.rand(batch, n_templates, 3, size, size, generator=g) * 2 - 1
    n_extra = max(int(n_references), 1) - 1
    out["references"], out["reference_poses"] = reference[:, None], R_ref[:, None]
    if n_extra > 0:
        extra_img = torch.rand(batch, n_extra, 3, size, size, generator=g) * 2 - 1
        extra_R = random_rotations(batch * n_extra, g).reshape(batch, n_extra, 3, 3)
        out["references"] = torch.cat([out["references"], extra_img], dim=1)
        out["reference_poses"] = torch.cat([out["reference_poses"], extra_R], dim=1)
    return {k: v.to(device) for k, v in out.items()}


def occlude_queries(batch: Dict[str, torch.Tensor], frac: float, seed: int = 2022):
    """Paste ONE axis-aligned rectangle of seeded uniform noise covering `frac` of the area over each query image (no reference counterpart:
    a stand-in for another object in front of the crop).  Returns (a new batch -- the same tensors, `query` replaced and `visibility` added --,
    visibility (B, S, S) f32: 0 inside the rectangle, 1 elsewhere; hip.op_pool_mask turns it into the latent mask).  The rectangle is as square
    as the size allows, its place drawn per sample; everything is drawn on the host from `seed`, whatever the batch's device."""
    if not (0.0 <= frac < 1.0):
        raise ValueError(f"occlude_queries: frac {frac!r} outside [0, 1)")
    query = batch["query"]
    B, Cq, Sh, Sw = query.shape
    g = torch.Generator().manual_seed(seed)
    rh = min(Sh, max(1, int(round((frac ** 0.5) * Sh)))) if frac > 0 else 0
    rw = min(Sw, max(1, int(round(frac * Sh * Sw / rh)))) if frac > 0 else 0
    occluded = query.detach().cpu().clone()
    visibility = torch.ones(B, Sh, Sw, dtype=torch.float32)
    for b in range(B):
        y0 = int(torch.randint(0, Sh - rh + 1, (1,), generator=g))
        x0 = int(torch.randint(0, Sw - rw + 1, (1,), generator=g))
        noise = torch.rand(Cq, rh, rw, generator=g) * 2 - 1
        occluded[b, :, y0:y0 + rh, x0:x0 + rw] = noise.to(occluded.dtype)
        visibility[b, y0:y0 + rh, x0:x0 + rw] = 0.0
    out = dict(batch)
    out["query"] = occluded.to(query.device)
    out["visibility"] = visibility.to(query.device)
    return out, out["visibility"]


def build_model(seed: int = 2022, compute_dtype="f32", bank_dtype="f32", device="cuda", u_net_dim: Optional[int] = None,
                save_dir: Optional[str] = None, template_parallel: bool = False, max_hypotheses_per_launch: int = 512, encoder: str = "template"):
    """encoder: "template" (template_base.yaml's FeatureExtractor), "vae" (vae_base.yaml's VAE_StableDiffusion at the SD-1.5 shapes,
    synthetic weights: images -> 4-channel latents -> the U-Net -> retrieval on the latents) or "stub" (none: the images are the embeddings)."""
    from .encoder import FeatureExtractor
    from .model import PoseConditional
    from .u_net import UNet
    from .weights import synth_init_
    cfg = TEMPLATE_BASE
    if encoder == "vae":
        from .vae import SD15_CONFIG, VAE_StableDiffusion
        enc = VAE_StableDiffusion(None, latent_dim=4, config=SD15_CONFIG, compute_dtype=compute_dtype).synth_init_(seed)
    elif encoder == "template":
        enc = FeatureExtractor(**cfg["u_net"]["encoder"], compute_dtype=compute_dtype)
        synth_init_(enc, seed, prefix="encoder.")
    elif encoder == "stub":            # no encoder: the U-Net and the scoring run on the 3-channel images themselves (loader / plumbing checks)
        enc = StubEncoder(3)
    else:
        raise ValueError(f"encoder {encoder!r}: 'template', 'vae' or 'stub'")
    unet = UNet(u_net_dim=u_net_dim or cfg["u_net"]["u_net_dim"], rot_representation_dim=6, encoder=enc,
                pose_mlp_name=cfg["u_net"]["pose_mlp_name"], compute_dtype=compute_dtype)
    # U-Net tensors are keyed without the "encoder." prefix; the encoder was initialised above
    from .weights import synth_tensor
    with torch.no_grad():
        for k, v in unet.state_dict().items():
            if not k.startswith("encoder."):
                v.copy_(synth_tensor(seed, k, tuple(v.shape)))
    model = PoseConditional(unet, cfg["optim_config"], cfg["testing_config"], save_dir, bank_dtype=bank_dtype,
                            template_parallel=template_parallel, max_hypotheses_per_launch=max_hypotheses_per_launch)
    return model.to(device).eval()


from .metrics import GeodesicError  # noqa: E402


def geodesic_deg(predR: torch.Tensor, gtR: torch.Tensor) -> torch.Tensor:
    rel = predR.double() @ gtR.double().transpose(-1, -2)
    cos = (rel.diagonal(dim1=-2, dim2=-1).sum(-1) - 1.0) / 2.0
    return torch.rad2deg(torch.acos(cos.clamp(-1.0, 1.0)))


@torch.no_grad()
def eval_geodesic(model, batch: Dict[str, torch.Tensor], thresholds=(15, 30), save_path: Optional[str] = None, visualize: bool = False,
                  errors_out: Optional[list] = None, refine_iters: int = 0, distinct_deg: Optional[float] = None, temperature: float = 1.0,
                  coarse_to_fine=None, multi_ref=None, robust=None):
    """The body of PoseConditional.eval_geodesic (model.py:268-376).  visualize (effective with a decoding encoder and model.save_dir only,
    model.py:269-274; needs batch["gt_templates"] (B, N, 3, S, S)): the three kinds of pictures and the video under save_dir/media
    (nope_amd/vis.py), and `vis_imgs` -- the full-size f16 grid of the retrieved picture -- in the saved predictions.  errors_out: a list that
    receives this batch's (B,) top-1 errors in degrees (run_split pools them over a split).  refine_iters > 0 (no reference counterpart): the
    retrieved candidates are refined below the grid spacing (PoseConditional.refine) and scored as well: the same metric keys under a
    "refined/" prefix, and `refined_relR` (B, k, 3, 3) in the saved predictions; at 0 nothing changes.  distinct_deg (no reference counterpart
    either; None: nothing changes): the distinct pose modes of the scores within that radius (hip.op_pose_modes at `temperature`, the batch's
    symmetry classes) are scored as well -- the same metric keys under "modes/", computed on the mode seeds, plus the batch means
    "modes/entropy" (nats) and "modes/n_modes"; with refine_iters > 0 the refinement starts from the mode seeds as well and reports under
    "modes_refined/"; the saved predictions gain `mode_idx`, `mode_mass` and `entropy`.  coarse_to_fine (no reference counterpart; None: nothing
    changes; True or a dict of PoseConditional.retrieve_coarse_to_fine's keyword arguments): the exhaustive path runs as always and the search
    in stages over the nested grid (nope_amd/search.py) runs next to it -- the same metric keys under "c2f/", computed on the search's
    nearest_idx, "c2f/evaluated_frac" (the share of the grid that got a U-Net pass, batch mean) and "c2f/top1_agree" (the share of queries
    whose top-1 is the exhaustive one); the saved predictions gain `c2f_similarity` and `c2f_idx`.  multi_ref (no reference counterpart; None:
    nothing changes; a dict of PoseConditional.retrieve_multi's keyword arguments, may be empty): the retrieval from ALL of
    batch["references"] (B, R, 3, S, S) with batch["reference_poses"] (B, R, 3, 3) runs next to the single-reference one -- the same
    metric keys under "multi/" and "multi/top1_agree"; the saved predictions gain `multi_similarity`.  Two keys of the dict are taken out here:
    "coarse_to_fine" (True or a dict of the search's keyword arguments): the multi-reference retrieval itself runs in stages
    (PoseConditional.retrieve_multi_coarse_to_fine, max_refs 1 unless given) and "multi/evaluated_frac" is added; "refine_iters" > 0: its
    candidates are refined, each through its nearest reference (refine_multi_from_feat), and scored under "multi_refined/".  robust (no
    reference counterpart; None: nothing changes; {"trim": t, "use_mask": bool}): the SAME bank is scored once more with the occlusion-robust
    score (hip.robust_similarity: the largest terms of a fraction t of the scored pixels dropped per hypothesis; with use_mask only the latent
    pixels whose cell of batch["visibility"] (B, S, S) f32 -- occlude_queries' plane -- is at least half visible are scored) -- the same metric
    keys under "robust/" and "robust/top1_agree"; the saved predictions gain `robust_similarity`.  No accuracy is claimed for it: the weights
    are synthetic."""
    visualize = bool(visualize) and model._decoder() is not None and model.save_dir is not None
    if visualize and "gt_templates" not in batch:
        raise ValueError('eval_geodesic(visualize=True) with a decoding encoder and save_dir needs batch["gt_templates"] (B, N, 3, S, S): '
                         "the template and retrieved pictures show them (model.py:217,331-333)")
    query, reference = batch["query"], batch["reference"]
    loss = model.forward(query, reference, batch["gt_relativeR"])
    if not visualize:
        similarity, nearest_idx, bank = model.generate_and_retrieve(query, reference, batch["all_relativeR"])
    else:
        from . import vis
        media, tag = os.path.join(model.save_dir, "media"), f"step{model.global_step}_rank{model.global_rank}"
        # the reconstruction under the ground-truth pose (model.py:284-306)
        _, pred_rgb = model.sample(reference=reference, relativeR=batch["gt_relativeR"])
        vis.save_png(vis.contact_sheet(vis.triptych(reference, query, pred_rgb, third_unnormalize=False))[0], os.path.join(media, f"reconst_{tag}.png"))
        # the bank has to be decoded: generate_templates + retrieval, the two calls generate_and_retrieve fuses (same arithmetic, same bits)
        bank, _, _ = model.generate_templates(reference=reference, all_relativeR=batch["all_relativeR"], gt_templates=batch["gt_templates"], visualize=True)
        similarity, nearest_idx = model.retrieval(query=query, template_feat=bank)
        # gt_templates[b, nearest_idx[b, 0]] (model.py:331-338): gathered by the kernel through the index, no look at it on the host
        retrieved = vis.triptych(reference, query, batch["gt_templates"], third_unnormalize=True, index=nearest_idx[:, 0])
        vis.save_png(vis.contact_sheet(retrieved)[0], os.path.join(media, f"retrieved_{tag}.png"))
    sym = batch.get("symmetry", torch.zeros(nearest_idx.shape[0], 1, dtype=torch.long, device=nearest_idx.device))
    # pred_R = template_poses[0][nearest_idx] -> GeodesicError (model.py:352-358, loss.py:78-115): gather + angle + symmetry branches as
    # one device launch (nope_op_geodesic); the grid of the first sample serves every query, as model.py:352 indexes it
    top1, metric = GeodesicError(list(thresholds)).from_indices(batch["template_poses"][:1], nearest_idx, batch["query_pose"], sym)
    if errors_out is not None:
        errors_out.append(top1)
    res = {"loss": float(loss)}
    res.update({k: float(v) for k, v in metric.items()})
    extra = {}
    if refine_iters > 0:
        ref = model.refine(query, reference, batch["all_relativeR"], nearest_idx, similarity, iters=refine_iters, template_poses=batch["template_poses"][:1])
        # pred_R (B, k, 3, 3) is a per-sample pose table for the same launch: rows 0 .. k - 1 of sample b
        _, refined = GeodesicError(list(thresholds))._topk_result(hip.op_geodesic(ref.pred_R, batch["query_pose"], sym))
        res.update({f"refined/{k}": float(v) for k, v in refined.items()})
        if save_path:
            extra["refined_relR"] = ref.relR.cpu().numpy()
    if distinct_deg is not None:
        modes = hip.op_pose_modes(similarity, batch["template_poses"][:1], sym, temperature=temperature, radius_deg=distinct_deg,
                                  max_modes=nearest_idx.shape[1], fill=True, want_prob=False)
        _, m_metric = GeodesicError(list(thresholds)).from_indices(batch["template_poses"][:1], modes.idx, batch["query_pose"], sym)
        res.update({f"modes/{k}": float(v) for k, v in m_metric.items()})
        res["modes/entropy"], res["modes/n_modes"] = float(modes.entropy.mean()), float(modes.n_modes.float().mean())
        if refine_iters > 0:
            ref = model.refine(query, reference, batch["all_relativeR"], modes.idx, similarity, iters=refine_iters, template_poses=batch["template_poses"][:1])
            _, refined = GeodesicError(list(thresholds))._topk_result(hip.op_geodesic(ref.pred_R, batch["query_pose"], sym))
            res.update({f"modes_refined/{k}": float(v) for k, v in refined.items()})
        if save_path:
            extra.update(mode_idx=modes.idx.cpu().numpy(), mode_mass=modes.mass.cpu().numpy(), entropy=modes.entropy.cpu().numpy())
    if coarse_to_fine is not None and coarse_to_fine is not False:
        c2f = model.retrieve_coarse_to_fine(query, reference, batch["all_relativeR"], batch["template_poses"][:1],
                                            **({} if coarse_to_fine is True else dict(coarse_to_fine)))
        _, c_metric = GeodesicError(list(thresholds)).from_indices(batch["template_poses"][:1], c2f.nearest_idx, batch["query_pose"], sym)
        res.update({f"c2f/{k}": float(v) for k, v in c_metric.items()})
        res["c2f/evaluated_frac"] = float(c2f.n_evaluated.float().mean()) / similarity.shape[1]
        res["c2f/top1_agree"] = float((c2f.nearest_idx[:, 0] == nearest_idx[:, 0]).float().mean())
        if save_path:
            extra.update(c2f_similarity=c2f.similarity.cpu().numpy(), c2f_idx=c2f.nearest_idx.cpu().numpy())
    if multi_ref is not None and multi_ref is not False:
        if "references" not in batch or "reference_poses" not in batch:
            raise ValueError('eval_geodesic(multi_ref=...) needs batch["references"] (B, R, 3, S, S) and batch["reference_poses"] (B, R, 3, 3)')
        mkw = {} if multi_ref is True else dict(multi_ref)
        m_c2f, m_refine = mkw.pop("coarse_to_fine", None), int(mkw.pop("refine_iters", 0))
        tpl = batch["template_poses"][:1]
        model._no_multi_ref_shards()
        q_feat, ref_feats = model._encode_multi(query, batch["references"])      # once: retrieval and refinement both start from the embeddings
        if m_c2f is not None and m_c2f is not False:       # the search in stages, every admitted pose from its max_refs nearest references
            mkw.pop("return_per_reference", None)
            if "dist_kind" in mkw:
                mkw["ref_dist_kind"] = mkw.pop("dist_kind")
            if mkw.get("max_refs") is None:
                mkw["max_refs"] = 1
            mr = model.retrieve_multi_coarse_to_fine_from_feat(q_feat, ref_feats, batch["reference_poses"], tpl, **mkw, **({} if m_c2f is True else dict(m_c2f)))
            res["multi/evaluated_frac"] = float(mr.n_evaluated.float().mean()) / similarity.shape[1]
        else:
            mr = model.retrieve_multi_from_feat(q_feat, ref_feats, batch["reference_poses"], tpl, **mkw)
        _, r_metric = GeodesicError(list(thresholds)).from_indices(tpl, mr.nearest_idx, batch["query_pose"], sym)
        res.update({f"multi/{k}": float(v) for k, v in r_metric.items()})
        res["multi/top1_agree"] = float((mr.nearest_idx[:, 0] == nearest_idx[:, 0]).float().mean())
        if m_refine > 0:                                   # each candidate refined through its nearest reference
            ref = model.refine_multi_from_feat(q_feat, ref_feats, batch["reference_poses"], tpl, mr.nearest_idx, n_refs=mkw.get("n_refs"), iters=m_refine)
            _, refined = GeodesicError(list(thresholds))._topk_result(hip.op_geodesic(ref.pred_R, batch["query_pose"], sym))
            res.update({f"multi_refined/{k}": float(v) for k, v in refined.items()})
        if save_path:
            extra.update(multi_similarity=mr.similarity.cpu().numpy())
    if robust is not None and robust is not False:
        rkw = dict(robust)
        use_mask, trim = bool(rkw.pop("use_mask", False)), float(rkw.pop("trim", 0.0))
        if rkw:
            raise TypeError(f"eval_geodesic(robust=...) got unexpected keys {sorted(rkw)}")
        q_feat = model.u_net.encoder.encode_image(query, mode="mode")
        mask = None
        if use_mask:
            if "visibility" not in batch:
                raise ValueError('eval_geodesic(robust={"use_mask": True}) needs batch["visibility"] (B, S, S) f32 (occlude_queries makes it)')
            mask = hip.op_pool_mask(batch["visibility"].float(), q_feat.shape[2:], 0.5)
        r_sim, r_idx = model.retrieval_from_feat(q_feat, bank, k=nearest_idx.shape[1], robust={"mask": mask, "trim": trim})
        _, r_metric = GeodesicError(list(thresholds)).from_indices(batch["template_poses"][:1], r_idx, batch["query_pose"], sym)
        res.update({f"robust/{k}": float(v) for k, v in r_metric.items()})
        res["robust/top1_agree"] = float((r_idx[:, 0] == nearest_idx[:, 0]).float().mean())
        if save_path:
            extra.update(robust_similarity=r_sim.cpu().numpy())
    if save_path:
        if visualize:       # model.py:334-339,367-375: the un-resized grid of the last picture
            extra["vis_imgs"] = hip.op_vis_grid(retrieved)[0].cpu().numpy()
        np.savez(save_path, **extra, query_pose=batch["query_pose"].cpu().numpy(), similarity=similarity.cpu().numpy())
    return similarity, nearest_idx, res


def run_split(model, dataset, batch_size: int = 1, limit: Optional[int] = None, visualize: bool = False, save_dir: Optional[str] = None,
              thresholds=(15, 30)) -> Dict[str, float]:
    """The test loop over one ShapeNet testing split: `dataset.load_batch` -> `eval_geodesic` per batch.  Returns the split's scores over ALL
    samples: accuracies weighted by sample (not a mean of per-batch percentages) and the median of the concatenated top-1 errors (not a mean
    of per-batch medians).  The ground-truth templates are decoded only when they are drawn (visualize)."""
    n = len(dataset) if limit is None else min(limit, len(dataset))
    errors = []
    for start in range(0, n, batch_size):
        batch = dataset.load_batch(list(range(start, min(start + batch_size, n))), with_templates=visualize)
        save = os.path.join(save_dir, "predictions", f"pred_step{start // batch_size}_rank{model.global_rank}") if save_dir else None
        eval_geodesic(model, batch, thresholds, save_path=save, visualize=visualize, errors_out=errors)
    errors = torch.cat([e.double().cpu() for e in errors]) if errors else torch.zeros(0, dtype=torch.float64)
    res = {f"accuracy_{t}": float((errors <= t).double().mean() * 100) if n else float("nan") for t in thresholds}
    res.update(median=float(errors.median()) if n else float("nan"), samples=n)
    return res


def main_dataset(a, ap):
    """`--data-root`: a testing split from disk."""
    from .dataset import ShapeNet
    if not a.id2cat:
        ap.error("--data-root needs --id2cat (the reference's src/utils/shapeNet_id2cat_v2.json)")
    if a.visualize and (a.encoder != "vae" or not a.save_dir):
        ap.error("--visualize needs --encoder vae (the template encoder decodes nothing, model.py:269-274) and --save-dir")
    device = hip.compute_device().type                    # ("cpu" only under tests/' interpreter build of the kernels)
    if device == "cuda" and not torch.cuda.is_available():
        raise SystemExit("nope_amd.harness needs an MI355X (no CPU fallback)")
    t0 = time.time()
    ds = ShapeNet(a.data_root, a.split, "upper", "rotation6d", fast_evaluation=a.fast, img_size=a.size or 256, level=2, id2cat=a.id2cat,
                  seed=a.seed, with_templates=a.visualize, pose_root=a.pose_root)
    model = build_model(a.seed, a.dtype, a.bank_dtype, device, u_net_dim=a.u_net_dim, save_dir=a.save_dir, encoder=a.encoder)
    res = run_split(model, ds, a.batch, a.limit, a.visualize, a.save_dir)
    if device == "cuda":
        torch.cuda.synchronize()
    res.update(dataloader=f"shapeNet_{a.split}", templates=len(ds.testing_indexes), seconds=time.time() - t0)
    print(json.dumps(res))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--templates", type=int, default=64)
    ap.add_argument("--size", type=int, default=None, help="image size (default: 128 for the synthetic batch, 256 for --data-root)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16x2", "bf16x3", "f16", "bf16"])
    ap.add_argument("--bank-dtype", default="f32", choices=["f32", "bf16", "f16"])
    ap.add_argument("--seed", type=int, default=2022)
    ap.add_argument("--category", default="synthetic")
    ap.add_argument("--save-dir", default=None)
    ap.add_argument("--pose-level", type=int, default=None, choices=[0, 1, 2, 3],
                    help="use the upper-hemisphere icosphere grid (26/91/341/1321 templates) instead of --templates random poses")
    ap.add_argument("--pose-root", default=None, help="directory with the reference's predefined_poses/*.npy")
    ap.add_argument("--encoder", default="template", choices=["template", "vae", "stub"],
                    help="vae: the Stable Diffusion VAE at the SD-1.5 shapes (synthetic weights) in place of the template encoder; "
                         "stub: no encoder, the images themselves are the embeddings (a check of the loader and the plumbing)")
    ap.add_argument("--visualize", action="store_true",
                    help="with --encoder vae and --save-dir: write the reconstruction / template / retrieved pictures, the video and vis_imgs")
    ap.add_argument("--data-root", default=None, help="a rendered ShapeNet root (cad_names.txt, images/, object_*_poses/): evaluate --split from disk")
    ap.add_argument("--split", default="bottle", help="with --data-root: the testing category")
    ap.add_argument("--id2cat", default=None, help="with --data-root: the reference's src/utils/shapeNet_id2cat_v2.json (synset id -> category)")
    ap.add_argument("--fast", action="store_true", help="with --data-root: fast_evaluation, the 26 level-0 viewpoints instead of the 341 of level 2")
    ap.add_argument("--limit", type=int, default=None, help="with --data-root: only the first N samples of the split")
    ap.add_argument("--u-net-dim", type=int, default=None, help="with --data-root: U-Net width (default: template_base.yaml's 192)")
    ap.add_argument("--refine", type=int, default=0, metavar="ITERS",
                    help="refine the retrieved poses with ITERS Gauss-Newton iterations through the U-Net and print their scores as well (refined/...)")
    ap.add_argument("--distinct-deg", type=float, default=None, metavar="D",
                    help="also score the distinct pose modes of the similarity within D degrees (modes/...: their seeds, the entropy, the mode count)")
    ap.add_argument("--temperature", type=float, default=1.0, metavar="T", help="with --distinct-deg: the softmax temperature, in score units")
    ap.add_argument("--coarse-to-fine", action="store_true",
                    help="with --pose-level: also retrieve in stages over the nested grid and print its scores (c2f/...: the metrics, the evaluated share, the agreement with the exhaustive top-1)")
    ap.add_argument("--c2f-seeds", type=int, default=3, metavar="M", help="with --coarse-to-fine: the best M poses of a stage seed the next")
    ap.add_argument("--references", type=int, default=1, metavar="R",
                    help="also retrieve from R posed reference views per object, fused (multi/...: the metrics, the agreement with the single-reference top-1)")
    ap.add_argument("--fusion", default="feature", choices=["feature", "score"], help="with --references: blend the predicted embeddings and score once, or average the score rows")
    ap.add_argument("--weighting", default="softmax", choices=["uniform", "softmax", "nearest"], help="with --references: the blend weights over the references")
    ap.add_argument("--max-refs", type=int, default=None, metavar="M",
                    help="with --references: generate every pose from its M nearest references only (M U-Net passes per pose whatever R is); "
                         "with --coarse-to-fine / --refine as well, the multi-reference retrieval runs in stages / its candidates are refined")
    ap.add_argument("--occlude", type=float, default=0.0, metavar="FRAC", help="paste a rectangle of seeded noise covering FRAC of each query image (occlude_queries)")
    ap.add_argument("--trim", type=float, default=0.0, metavar="FRAC",
                    help="also score the bank with the occlusion-robust score, the largest terms of FRAC of the scored pixels dropped per hypothesis (robust/...)")
    ap.add_argument("--use-mask", action="store_true", help="with --occlude: the robust score reads only the latent pixels the rectangle leaves at least half visible")
    ap.add_argument("--tau-deg", type=float, default=30.0, metavar="D", help="with --weighting softmax: the temperature, degrees of pose distance")
    a = ap.parse_args(argv)
    if not 1 <= a.references <= hip.MULTIREF_MAX_REFS:
        ap.error(f"--references: 1 .. {hip.MULTIREF_MAX_REFS}")
    if a.max_refs is not None and not 1 <= a.max_refs <= a.references:
        ap.error("--max-refs: 1 .. --references")
    if not 0.0 <= a.occlude < 1.0 or not 0.0 <= a.trim < 1.0:
        ap.error("--occlude / --trim: a fraction in [0, 1)")
    if a.use_mask and a.occlude <= 0.0:
        ap.error("--use-mask needs --occlude (the mask is the rectangle's complement)")
    if a.data_root:
        if a.refine or a.distinct_deg is not None or a.coarse_to_fine or a.references > 1 or a.occlude or a.trim:
            ap.error("--refine / --distinct-deg / --coarse-to-fine / --references / --occlude / --trim apply to the synthetic batch (a split's pooled scores carry none of them)")
        return main_dataset(a, ap)
    a.size = a.size or 128
    if a.coarse_to_fine and a.pose_level is None:
        ap.error("--coarse-to-fine needs --pose-level (a nested icosphere grid; random poses have no levels)")
    if a.visualize and (a.encoder != "vae" or not a.save_dir):
        ap.error("--visualize needs --encoder vae (the template encoder decodes nothing, model.py:269-274) and --save-dir")
    if not torch.cuda.is_available():
        raise SystemExit("nope_amd.harness needs an MI355X (no CPU fallback)")
    model = build_model(a.seed, a.dtype, a.bank_dtype, "cuda", save_dir=a.save_dir, encoder=a.encoder)
    batches = {f"shapeNet_{a.category}": synthetic_batch(a.batch, a.templates, a.size, a.seed, "cuda", pose_level=a.pose_level,
                                                                  pose_root=a.pose_root, gt_templates=a.visualize,
                                                                  n_references=a.references)}
    c2f = None
    if a.coarse_to_fine:
        from .poses import grid_stages
        c2f = dict(seeds=a.c2f_seeds, stage_of=grid_stages(a.pose_level, "upper", root=a.pose_root))
    multi = None
    if a.references > 1 and a.max_refs is None and (a.coarse_to_fine or a.refine):
        print("note: --coarse-to-fine / --refine apply to the single-reference retrieval only; add --max-refs M to run them through the "
              "references as well (multi/evaluated_frac, multi_refined/...)", file=sys.stderr)
    if a.references > 1:
        multi = dict(fusion=a.fusion, weighting=a.weighting, tau_deg=a.tau_deg)
        if a.max_refs is not None:          # the sparse path and, through it, the stages and the refinement from several references
            multi.update(max_refs=a.max_refs, coarse_to_fine=c2f, refine_iters=a.refine)
    robust = {"trim": a.trim, "use_mask": a.use_mask} if (a.trim > 0.0 or a.use_mask) else None
    for name, batch in batches.items():                         # test_step, model.py:550-565
        if a.occlude > 0.0:
            batch, _ = occlude_queries(batch, a.occlude, a.seed)
        t0 = time.time()
        save = os.path.join(a.save_dir, "predictions", f"pred_step0_rank{model.global_rank}") if a.save_dir else None
        sim, idx, res = eval_geodesic(model, batch, save_path=save, visualize=a.visualize, refine_iters=a.refine, distinct_deg=a.distinct_deg,
                                      temperature=a.temperature, coarse_to_fine=c2f,
                                      multi_ref=multi, robust=robust)
        torch.cuda.synchronize()
        res.update(dataloader=name, seconds=time.time() - t0, nearest_idx=idx.tolist())
        print(json.dumps(res))


if __name__ == "__main__":
    main()
