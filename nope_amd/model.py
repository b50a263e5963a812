"""`PoseConditional` -- the task module of the hot path, mirroring the reference's call
surface (src/model/model.py:32-266): `forward`, `sample`, `generate_templates`, `retrieval`
with the same arguments and return tuples, on top of the HIP U-Net and scoring kernels.

Differences in *schedule*, none in arithmetic:
  * `generate_templates` encodes the reference image once (the reference re-encodes it for
    every template, model.py:115 via :219) and evaluates all N pose hypotheses as batched
    U-Net launches writing straight into the (B,N,C,h,w) bank;
  * `retrieval` never materialises the N-fold repeated query (model.py:258);
  * top-k uses "descending score, ties -> lowest index" (torch.topk leaves tie order
    unspecified);
  * with `template_parallel=True` under torch.distributed each rank generates and scores only
    its slice of the template axis and the scores are all-gathered (nope_amd/dist.py).
Lightning-specific members (optimizers, wandb logging) are out of scope and are not provided; the visualisation outputs
(PNG contact sheets, video, `vis_imgs`) are written by nope_amd/vis.py.
The evaluation entry points -- `eval_geodesic`, `eval_vsd` (T-LESS, on the device: nope_amd/vsd.py), `load_mesh`,
`validation_step`, `test_step` -- return their scores instead of logging them; `eval_bop` / `load_models_info` (the BOP benchmark's other
errors, nope_amd/bop.py; no reference counterpart) do the same.
"""
from __future__ import annotations

import inspect
import os
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import dist as ndist
from . import hip


class RefineResult(NamedTuple):
    """What PoseConditional.refine_from_feat returns (its docstring has the shapes)."""
    relR: torch.Tensor
    rot6d: torch.Tensor
    score: torch.Tensor
    score_init: torch.Tensor
    accepted: torch.Tensor
    order: torch.Tensor
    costs: torch.Tensor
    status: torch.Tensor
    trajectory: torch.Tensor
    pred_R: Optional[torch.Tensor]


class MultiRefResult(NamedTuple):
    """What PoseConditional.retrieve_multi_from_feat returns: similarity (B,N) f32, the fused row; nearest_idx (B,k) int64; weights (B,R,N)
    f32, the blend weights (NaN for a sample whose reference poses or count were invalid: its fused row is NaN too); per_reference (B,R,N)
    f32, the single-reference scores, or None; bank (B,R,N,C,h,w).  With max_refs = M (the sparse path): weights, per_reference (the per-slot
    rows) and bank have M in place of R, and src (B,M,N) int32 names the reference each slot was generated from (None on the dense path)."""
    similarity: torch.Tensor
    nearest_idx: torch.Tensor
    weights: torch.Tensor
    per_reference: Optional[torch.Tensor]
    bank: torch.Tensor
    src: Optional[torch.Tensor] = None


def _cfg_get(cfg, key, default=None):
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class PoseConditional(nn.Module):
    def __init__(self, u_net, optim_config=None, testing_config=None, save_dir=None, bank_dtype="f32",
                 max_hypotheses_per_launch=512, template_parallel=False, two_stream_below=None, pipeline_encoders=False, **kwargs):
        super().__init__()
        self.u_net = u_net
        self.save_dir = save_dir
        self.lr = _cfg_get(optim_config, "lr", 5e-5)
        self.weight_decay = _cfg_get(optim_config, "weight_decay", 0.0005)
        self.warm_up_steps = _cfg_get(optim_config, "warm_up_steps", 500)
        self.use_inv_deltaR = _cfg_get(optim_config, "use_inv_deltaR", True)
        self.loss_type = _cfg_get(optim_config, "loss_type", "l1")
        self.testing_config = testing_config
        self.similarity_metric = _cfg_get(testing_config, "similarity_metric", "l2")
        self.bank_dtype = bank_dtype
        self.max_hyp = int(max_hypotheses_per_launch)
        self.template_parallel = bool(template_parallel)
        # generate_and_retrieve: both encoder passes on the side stream WITHOUT waiting for what the current stream has queued, so that the
        # (launch-latency-bound, few CUs wide) encoder passes of query k + 1 run in the gaps of query k's U-Net instead of in front of their
        # own.  Only for callers whose `query` / `reference` tensors are complete when the call is made (not still being produced by work
        # queued on the current stream): results are the same bits, consecutive calls overlap on the device.  NOPE_PIPELINE_ENCODERS overrides.
        env = os.environ.get("NOPE_PIPELINE_ENCODERS")
        self.pipeline_encoders = bool(int(env)) if env is not None else bool(pipeline_encoders)
        # Single-query banks of at most this many templates (the reference's 26 / 91-template grids) are generated as two half
        # batches on two HIP streams: with a few dozen hypotheses most launches of a forward have fewer tiles than the chip has
        # workgroup slots, and two independent launch sequences fill each other's idle CUs (NOPE_TWO_STREAM_BELOW overrides; 0 = off).
        env = os.environ.get("NOPE_TWO_STREAM_BELOW")
        self.two_stream_below = int(env) if env is not None else (int(two_stream_below) if two_stream_below is not None else 0)
        self.global_step = 0
        self.global_rank = ndist.world()[0]
        if save_dir is not None:    # model.py:63-66
            os.makedirs(os.path.join(save_dir, "media"), exist_ok=True)
            os.makedirs(os.path.join(save_dir, "predictions"), exist_ok=True)
            self.log_dir = os.path.join(save_dir, "predictions")

    # ---- model.py:96-111 ------------------------------------------------------------------
    def compute_loss(self, pred, gt):
        d = (pred - gt).abs() if self.loss_type == "l1" else (pred - gt) ** 2
        return d.flatten(1).mean(dim=1).mean()

    @torch.no_grad()
    def forward(self, query, reference, relativeR):
        enc = self.u_net.encoder
        query_feat = enc.encode_image(query)
        reference_feat = enc.encode_image(reference, mode="mode")
        pred_query_feat = self.u_net(reference_feat, relativeR)
        return self.compute_loss(pred_query_feat, query_feat)

    # ---- model.py:113-124 -------------------------------------------------------------------
    def _decoder(self):
        """The encoder's `decode_latent` (the VAE, nope_amd/vae.py), or None (the template encoder has none, model.py:117-123)."""
        dec = getattr(self.u_net.encoder, "decode_latent", None)
        return dec if callable(dec) else None

    @torch.no_grad()
    def sample(self, reference, relativeR):
        reference_feat = self.u_net.encoder.encode_image(reference, mode="mode")
        pred_query_feat = self.u_net(reference_feat, relativeR)
        dec = self._decoder()
        if dec is None:
            return pred_query_feat, None
        # unnormalize_to_zero_to_one(decode_latent(pred)), model.py:117-123
        if "unnormalize" in inspect.signature(dec).parameters:      # nope_amd's VAE: (x + 1) / 2 folded into its output conv
            return pred_query_feat, dec(pred_query_feat, unnormalize=True)
        return pred_query_feat, (dec(pred_query_feat) + 1) / 2      # another encoder's decode_latent, as the reference applies it

    # ---- model.py:193-252 -----------------------------------------------------------------------
    @torch.no_grad()
    def generate_templates(self, reference, all_relativeR, gt_templates=None, visualize=False):
        """reference (B,3,S,S); all_relativeR (B,N,6) -> (pred_feat_templates (B,N',C,S/8,S/8),
        pred_templates, vid_path).  N' = N, or this rank's slice of N under `template_parallel`.  pred_templates: with an encoder that has
        `decode_latent` (the VAE), the decoded templates (B,N',3,S,S) f32 (model.py:199-206,221-224), decoded on the device in chunks of
        bounded workspace; else None.  visualize=True (model.py:214-249; needs gt_templates (B,N,3,S,S), a decoding encoder and save_dir):
        one picture per template, media/template{i}_rank{rank}.png with i the global template index -- unnormalize(reference) |
        unnormalize(gt_templates[:, i]) | unnormalize(pred_templates[:, i]) at 64 x 64 (pred_templates is the decoder's output in [-1, 1];
        the reference shows its `sample`'s unnormalize_to_zero_to_one(decode), model.py:219-226: the same picture) -- and their video, whose path is the third value (None
        otherwise; see nope_amd/vis.py)."""
        if visualize and gt_templates is None:
            raise ValueError("generate_templates(visualize=True) needs gt_templates (model.py:217)")
        reference_feat = self.u_net.encoder.encode_image(reference, mode="mode")   # hoisted: once, not N times
        bank = self.generate_templates_from_feat(reference_feat, all_relativeR)
        dec = self._decoder()
        if dec is None:
            return bank, None, None
        B, n = bank.shape[:2]
        lat = torch.Tensor._make_subclass(torch.Tensor, bank, False) if isinstance(bank, ndist.ShardedBank) else bank
        lat = lat.reshape(B * n, *bank.shape[2:])
        if lat.dtype != torch.float32:
            lat = lat.float()         # (16-bit banks: the decoder reads f32 latents)
        rgb = dec(lat)                # (an empty bank decodes to (0, 3, S, S))
        rgb = rgb.reshape(B, n, *rgb.shape[1:])
        vid_path = None
        if visualize and self.save_dir is not None:
            lo = bank.shard[0] if isinstance(bank, ndist.ShardedBank) else 0
            vid_path = self._save_template_pictures(reference, gt_templates[:, lo:lo + n], rgb, lo)
        return bank, rgb, vid_path

    def _save_template_pictures(self, reference, gt_templates, pred_templates, first):
        """model.py:214-249 for templates [first, first + n): every frame's PNG bytes from chunked launches over the frame axis (a chunk is copied out before the next is
        made), one file per template, and the frames as a video.  Returns the video's path (None without frames)."""
        from . import vis
        media = os.path.join(self.save_dir, "media")
        frames = []                   # on the host; the device holds one chunk of sheets at a time
        for f0, chunk in vis.contact_sheet_chunks(vis.triptych(reference, gt_templates, pred_templates, third_unnormalize=True)):
            for j, frame in enumerate(chunk.cpu().numpy()):
                vis.save_png(frame, os.path.join(media, f"template{first + f0 + j}_rank{self.global_rank}.png"))
                frames.append(frame)
        if not frames:
            return None
        return vis.write_video(frames, os.path.join(media, f"video_step{self.global_step}_rank{self.global_rank}"))

    @torch.no_grad()
    def generate_templates_from_feat(self, reference_feat, all_relativeR, defer_range_check=False):
        """defer_range_check (f16x2): the caller finishes the U-Net's range check itself (generate_and_retrieve: after scoring)."""
        out = self._generate_templates_from_feat(reference_feat, all_relativeR)
        if not defer_range_check:
            self.u_net.finish_range_check()        # (repeats the forwards in place when a layer left its accurate window: hip.UNetHandle)
        return out

    def _generate_templates_from_feat(self, reference_feat, all_relativeR):
        B, N = all_relativeR.shape[:2]
        lo, hi, ws = 0, N, 1
        if self.template_parallel:
            rank, ws = ndist.world()
            lo, hi = ndist.shard_range(N, rank, ws)
        poses = all_relativeR[:, lo:hi].contiguous().float()
        n = hi - lo
        C, h, w = self.u_net.channels, reference_feat.shape[2], reference_feat.shape[3]   # latent_dim, model.py:207-210
        bank = torch.empty((B, n, C, h, w), dtype=hip.torch_dtype(hip.dtype_code(self.bank_dtype)),
                           device=reference_feat.device)
        out = bank
        if ws > 1:
            # a sharded bank is a ShardedBank: it carries its placement (lo, hi, N) in its type, so retrieval gathers exactly the banks
            # made here, never a caller-supplied tensor that merely has the same local size
            out = ndist.ShardedBank(bank, lo, hi, N)
        if n == 0:                  # more ranks than templates: this rank still takes part in the all-gather
            return out
        if B == 1 and 2 <= n <= self.two_stream_below and reference_feat.is_cuda:
            # (off by default.  Splitting n changes the GEMM row count and with it the launch plan: the halves agree with the
            #  single-batch result to rounding, not bit for bit -- tests/test_gpu_configs.py::test_two_stream_split_close_to_single_batch)
            n_first = (n + 1) // 2
            with hip.overlap_stream(reference_feat) as side:
                self.u_net.forward_hypotheses(reference_feat, poses[:, n_first:].contiguous(), out=bank[:, n_first:], out_dtype=self.bank_dtype, defer_range_check=True)
            self.u_net.forward_hypotheses(reference_feat, poses[:, :n_first].contiguous(), out=bank[:, :n_first], out_dtype=self.bank_dtype, defer_range_check=True)
            side.join(bank)
            return out
        if n <= self.max_hyp:
            bs = max(1, self.max_hyp // n)
            for b0 in range(0, B, bs):
                self.u_net.forward_hypotheses(reference_feat[b0:b0 + bs], poses[b0:b0 + bs], out=bank[b0:b0 + bs],
                                              out_dtype=self.bank_dtype, defer_range_check=True)
        else:
            for b in range(B):
                for s in range(0, n, self.max_hyp):
                    e = min(n, s + self.max_hyp)
                    self.u_net.forward_hypotheses(reference_feat[b:b + 1], poses[b:b + 1, s:e],
                                                  out=bank[b:b + 1, s:e], out_dtype=self.bank_dtype, defer_range_check=True)
        return out

    # ---- model.py:254-266 ----------------------------------------------------------------------------
    @torch.no_grad()
    def retrieval(self, query, template_feat, shard=None):
        if self.similarity_metric != "l2":
            return None                   # the reference implements only "l2" (model.py:256,266)
        query_feat = self.u_net.encoder.encode_image(query, mode="mode")
        return self.retrieval_from_feat(query_feat, template_feat, shard=shard)

    # ---- occlusion-robust scoring (no reference counterpart: DESIGN.md section 4.14) -----------------------------------------------------
    def _score(self, query_feat, bank, robust, **kw):
        """The score row of every retrieval: hip.similarity -- or, with robust = {"mask": (B,h,w) uint8|bool tensor or None, "trim": float},
        hip.robust_similarity.  robust=None is today's call, unchanged."""
        if robust is None:
            return hip.similarity(query_feat, bank, **kw)
        unknown = sorted(set(robust) - {"mask", "trim"})
        if unknown:
            raise TypeError(f"robust: unexpected keys {unknown} (expected 'mask' and / or 'trim')")
        return hip.robust_similarity(query_feat, bank, robust.get("mask"), robust.get("trim", 0.0), **kw)

    def _no_robust_shards(self, robust):
        if robust is not None and self.template_parallel and ndist.world()[1] > 1:
            raise NotImplementedError("robust scoring under template_parallel with more than one rank: sharded robust banks are not built")

    @staticmethod
    def _no_robust_multi(robust):
        if robust is not None:
            raise NotImplementedError("robust scoring with the multi-reference methods: the fused scoring kernel has no masked / trimmed form")

    @torch.no_grad()
    def retrieve_robust(self, query, reference, all_relativeR, mask=None, trim=0.0):
        """generate_and_retrieve with the occlusion-robust score (hip.robust_similarity; include/nope_hip.h: nope_robust_similarity):
        (similarity, nearest_idx, bank).  mask (B,h,w) uint8|bool at the latent size or None -- the pixels of the query that show the object
        (hip.op_pool_mask makes it from an alpha or visibility plane) --, trim in [0, 1): the fraction of the scored pixels whose largest
        terms are dropped per hypothesis.  The f16x2 range-check re-score is the robust score as well.  No default is tuned and no accuracy
        is claimed: there are no trained weights."""
        if self.similarity_metric != "l2":
            return None
        return self._encode_generate_retrieve(query, reference, all_relativeR, robust={"mask": mask, "trim": trim})[:3]

    # ---- model.py:313,323 (the two calls eval_geodesic makes back to back) --------------------------------
    @torch.no_grad()
    def generate_and_retrieve(self, query, reference, all_relativeR):
        """`generate_templates(reference, all_relativeR)` followed by `retrieval(query, bank)` as one call,
        returning (similarity, nearest_idx, bank) -- the same arithmetic in the same order, bit-identical results.  It never decodes the
        bank, with a VAE encoder either: retrieval needs the latents only (generate_templates returns the decoded templates).  The query does not depend on
        the bank, so its encoder pass (launch-latency bound, a few CUs wide) is issued on a second HIP
        stream and runs underneath the reference encoder and the first U-Net kernels."""
        if self.similarity_metric != "l2":
            return None
        return self._encode_generate_retrieve(query, reference, all_relativeR)[:3]

    def _encode_generate_retrieve(self, query, reference, all_relativeR, robust=None):
        """The body of generate_and_retrieve; also hands out the two embeddings (predict_pose refines on them)."""
        self._no_robust_shards(robust)
        if self.pipeline_encoders and query.is_cuda:
            with hip.overlap_stream(query, wait_current=False) as side:
                reference_feat = self.u_net.encoder.encode_image(reference, mode="mode")
                ref_done = side.mark()
                query_feat = self.u_net.encoder.encode_image(query, mode="mode")
            side.join_at(ref_done, reference_feat)          # the U-Net waits for the reference's pass only
        else:
            with hip.overlap_stream(query) as side:
                query_feat = self.u_net.encoder.encode_image(query, mode="mode")
            reference_feat = self.u_net.encoder.encode_image(reference, mode="mode")
        # (a sharded step finishes the check BEFORE its collective: every rank must enter the score all-gather exactly once, and whether a
        #  forward is repeated is a per-rank fact)
        # (the handle's "repeat" behaviour only -- in its "poison" behaviour no host look is needed at all: an out-of-range bank is NaN, and so are its scores)
        defer = not (self.template_parallel and ndist.world()[1] > 1)
        bank = self.generate_templates_from_feat(reference_feat, all_relativeR, defer_range_check=defer)
        side.join(query_feat)
        similarity, nearest_idx = self.retrieval_from_feat(query_feat, bank, robust=robust)
        # f16x2: the U-Net's activation-range check, at the END of the step -- one stream synchronisation where the results are read anyway.
        # When a layer had left its accurate window the forwards were just repeated into the same bank: score and rank again.
        if defer and self.u_net.finish_range_check():
            similarity, nearest_idx = self.retrieval_from_feat(query_feat, bank, robust=robust)
        return similarity, nearest_idx, bank, query_feat, reference_feat

    @torch.no_grad()
    def retrieval_topk_from_feat(self, query_feat, template_feat, k=5, shard=None, robust=None):
        """The top-k only -- (values (B,k), nearest_idx (B,k)) -- for callers that do not keep the full similarity: under `template_parallel` every
        rank ranks its own slice and only the (B, k) (score, global index) pairs are all-gathered and merged (north_star's "all-gather of
        per-shard top-k"; tie rule of model.py:265 as everywhere: lowest global index).  Same indices as `retrieval_from_feat`.
        robust: as retrieval_from_feat."""
        self._no_robust_shards(robust)
        sl = (template_feat.shard if isinstance(template_feat, ndist.ShardedBank) else None) if shard is None else (shard or None)
        if not (self.template_parallel and sl is not None):
            if self.template_parallel and shard is None and ndist.world()[1] > 1:
                raise hip.NopeError("template_parallel: this bank is a plain tensor without a shard placement: pass shard=(lo, hi, n_total) or shard=False")
            sim = self._score(query_feat, template_feat, robust)
            return hip.topk(sim, k)
        B, n_local = query_feat.shape[0], template_feat.shape[1]
        kl = min(k, n_local)
        if kl > 0:
            vals, idx = hip.topk(self._score(query_feat, template_feat, robust), kl)
            idx = idx + sl[0]
        else:
            vals = torch.empty((B, 0), dtype=torch.float32, device=query_feat.device)
            idx = torch.empty((B, 0), dtype=torch.int64, device=query_feat.device)
        return ndist.all_gather_topk_pairs(vals, idx, k)

    @torch.no_grad()
    def retrieval_from_feat(self, query_feat, template_feat, k=5, shard=None, robust=None):
        """`shard` = (lo, hi, N): this rank's slice [lo, hi) of the N templates; `shard=False`: the bank is COMPLETE on this rank
        (e.g. loaded from disk on every rank) and is scored locally without a collective.  Banks made by `generate_templates`
        are `nope_amd.dist.ShardedBank`s and carry their placement themselves; a bank that went through another op since (`.to()`,
        a slice, `torch.cat`, save / load) is a plain tensor again: under `template_parallel` with more than one rank that raises --
        scoring only a local slice while the other ranks wait in the collective would return rank-local indices without an error.
        robust (None: the reference's score, every output as without the argument): {"mask": (B,h,w) uint8|bool tensor or None, "trim":
        float in [0, 1)} scores with hip.robust_similarity instead; the row feeds hip.topk, pose_distribution and
        the coarse-to-fine commit unchanged.  NotImplementedError under template_parallel with more than one rank."""
        self._no_robust_shards(robust)
        sl = (template_feat.shard if isinstance(template_feat, ndist.ShardedBank) else None) if shard is None else (shard or None)
        if self.template_parallel and sl is None and shard is None and ndist.world()[1] > 1:
            raise hip.NopeError("template_parallel: this bank is a plain tensor, not a ShardedBank with a shard placement (it was not made by generate_templates, or was "
                                "copied / sliced since): pass shard=(lo, hi, n_total), or shard=False for a bank that is complete on every rank")
        if self.template_parallel and sl is not None:
            if sl[1] - sl[0] != template_feat.shape[1]:
                raise hip.NopeError(f"shard {tuple(sl)} does not match the bank's {template_feat.shape[1]} local templates")
            B, n_local = query_feat.shape[0], template_feat.shape[1]
            send, _ = ndist.gather_buffers(B, sl[2], query_feat.device)
            if n_local > 0:          # this rank's columns go straight into the collective's send buffer
                self._score(query_feat, template_feat, robust, out=send, col_offset=0)
            if ndist.world()[1] > 1 and k <= sl[2]:
                # scoring -> ONE collective -> ONE kernel (un-pad into an owned (B, N) similarity + top-k): nope_gather_topk
                return ndist.all_gather_scores_topk(n_local, sl[2], B, query_feat.device, k)
            similarity = ndist.all_gather_scores(send[:, :n_local], sl[2])
        else:
            similarity = self._score(query_feat, template_feat, robust)
        _, nearest_idx = hip.topk(similarity, k)
        return similarity, nearest_idx

    # ---- sub-grid refinement (no reference counterpart: DESIGN.md section 4.9) --------------------------------------------------------
    def _forward_poses(self, reference_feat, poses, out):
        """out (B,n,C,h,w) f32 = u_net(reference_feat[b], poses[b, i]), chunked by max_hypotheses_per_launch as _generate_templates_from_feat
        chunks a bank.  The range check (f16x2) is NOT deferred: the refinement rewrites `poses` before the step ends, and a deferred
        repeat would replay the forward on the rewritten poses."""
        B, n = poses.shape[:2]
        if n <= self.max_hyp:
            bs = max(1, self.max_hyp // n)
            for b0 in range(0, B, bs):
                self.u_net.forward_hypotheses(reference_feat[b0:b0 + bs], poses[b0:b0 + bs], out=out[b0:b0 + bs], defer_range_check=False)
        else:
            for b in range(B):
                for s in range(0, n, self.max_hyp):
                    e = min(n, s + self.max_hyp)
                    self.u_net.forward_hypotheses(reference_feat[b:b + 1], poses[b:b + 1, s:e], out=out[b:b + 1, s:e], defer_range_check=False)
        return out

    @torch.no_grad()
    def refine_from_feat(self, query_feat, reference_feat, all_relativeR, nearest_idx, similarity, iters=3, fd_step=1e-2, max_step_deg=10.0,
                         damping=1e-6, template_poses=None):
        """Gauss-Newton on SO(3) from the k retrieved candidates (include/nope_hip.h: nope_op_refine_*): per iteration ONE U-Net pass over
        seven poses per candidate (the pose and its six central-difference neighbours), the 3x3 normal equations of
        || u_net(reference_feat, dR) - query_feat ||^2 and a damped, clamped tangent step; then the reference's score (model.py:257-262) of
        the refined poses decides, per candidate, between the refined pose (strictly better) and the grid pose.  Nothing is read by the
        host (under f16x2 in "repeat" mode: the range checks of the forwards).
        query_feat, reference_feat (B,C,h,w) f32; all_relativeR (B,N,6); nearest_idx (B,k); similarity (B,N) as `retrieval` returns them.
        Returns a RefineResult, every per-candidate tensor in the final order (descending final score, ties -> the lower retrieval rank):
        relR (B,k,3,3) f64, rot6d (B,k,6) f32, score, score_init (B,k) f32, accepted (B,k) bool, order (B,k) int64 (retrieval rank of each
        entry), costs (iters,B,k) f64 (r^T r at the START of each iteration, in retrieval order), status (iters,B,k) int32 (hip.REFINE_*),
        trajectory (iters+1,B,k,3,3) f64 (dR before the first and after every step, retrieval order) and, with template_poses (B|1,N,3,3),
        pred_R (B,k,3,3) f64 = (dR dR_init^T) template_poses[nearest_idx]."""
        query_feat, reference_feat = query_feat.float().contiguous(), reference_feat.float().contiguous()
        return self._refine(query_feat, lambda poses, out: self._forward_poses(reference_feat, poses, out), all_relativeR, nearest_idx, nearest_idx,
                            similarity, iters, fd_step, max_step_deg, damping, template_poses)

    def _refine(self, query_feat, forward, rows, row_idx, nearest_idx, similarity, iters, fd_step, max_step_deg, damping, template_poses):
        """The loop of refine_from_feat / refine_multi_from_feat.  forward(poses (B,n,6), out (B,n,C,h,w)) fills `out` with the U-Net's maps of
        `poses`, n = 7k (candidate-major: the pose and its six neighbours) or k; rows[b, row_idx[b, j]] is candidate j's starting pose;
        similarity (B,N) holds the baseline score at nearest_idx -- or is None: the baseline is then the score of slot 0 of each group of
        seven in the FIRST iteration's forward, the starting pose through the same source as every later pass."""
        import math
        if iters < 1:
            raise ValueError("refine_from_feat: iters >= 1 (predict_pose(refine_iters=0) is the unrefined answer)")
        B, k = nearest_idx.shape
        C, h, w = query_feat.shape[1:]
        dR, dR0, poses, _ = hip.op_refine_init(rows, row_idx, fd_step)
        dev = dR.device
        maps = torch.empty((B, 7 * k, C, h, w), dtype=torch.float32, device=dev)
        ne = torch.empty((iters, B, k, 10), dtype=torch.float64, device=dev)
        status = torch.empty((iters, B, k), dtype=torch.int32, device=dev)
        traj = torch.empty((iters + 1, B, k, 3, 3), dtype=torch.float64, device=dev)
        ws = torch.empty(max(8, int(hip.lib().dll.nope_op_refine_normal_eq_workspace_bytes(B, k, h, w))) // 8, dtype=torch.float64, device=dev)
        traj[0].copy_(dR)
        for it in range(iters):
            forward(poses, maps)
            if similarity is None:
                base_score = hip.similarity(query_feat, maps.view(B, k, 7, C, h, w)[:, :, 0].contiguous())
                similarity = torch.full((B, template_poses.shape[1]), float("-inf"), dtype=torch.float32, device=dev)
                hip.op_c2f_commit(base_score, nearest_idx.to(torch.int32), similarity)
            hip.op_refine_normal_eq(query_feat, maps, fd_step, out=ne[it], workspace=ws)
            hip.op_refine_step(ne[it], dR, poses, fd_step, math.radians(max_step_deg), damping, status=status[it])
            traj[it + 1].copy_(dR)
        base = poses.view(B, k, 7, 6)[:, :, 0].contiguous()
        final_maps = forward(base, torch.empty((B, k, C, h, w), dtype=torch.float32, device=dev))
        score = hip.similarity(query_feat, final_maps)
        r = hip.op_refine_select(dR, dR0, score, similarity, nearest_idx, template_poses)
        return RefineResult(relR=r.dR, rot6d=r.rot6d, score=r.score, score_init=r.score_init, accepted=r.accepted, order=r.order,
                            costs=ne[..., 9], status=status, trajectory=traj, pred_R=r.pred_R)

    @torch.no_grad()
    def refine(self, query, reference, all_relativeR, nearest_idx, similarity, **kw):
        """Encode both images, then refine_from_feat (same keyword arguments)."""
        enc = self.u_net.encoder
        query_feat = enc.encode_image(query, mode="mode")
        reference_feat = enc.encode_image(reference, mode="mode")
        return self.refine_from_feat(query_feat, reference_feat, all_relativeR, nearest_idx, similarity, **kw)

    @torch.no_grad()
    def pose_distribution(self, similarity, template_poses, symmetry=None, temperature=1.0, radius_deg=15.0, max_modes=5):
        """The retrieval scores as a distribution over the template grid, and its distinct modes (hip.op_pose_modes, DESIGN.md section
        4.10): a PoseModes with prob (B,N), entropy (B,) in nats, and per mode idx / score / mass / count (B,max_modes) and n_modes (B,).
        A symmetric or otherwise ambiguous object shows as several modes of comparable mass and a high entropy.  similarity (B,N) as
        `retrieval` returns it (under template_parallel: the full matrix every rank holds), template_poses (B|1,N,3,3), symmetry (B,) in
        {0,1,2} (loss.py's classes).  `temperature` is in SCORE units, and a score is a sum over the h*w latent pixels (model.py:257-262),
        so the useful scale grows with the latent size.  No default here is tuned -- neither the temperature nor radius_deg (choose it
        from the grid: above its vertex spacing): there are no trained weights to tune them on."""
        return hip.op_pose_modes(similarity, template_poses, symmetry, temperature=temperature, radius_deg=radius_deg, max_modes=max_modes)

    # ---- coarse-to-fine retrieval (no reference counterpart: DESIGN.md section 4.11) ----------------------------------------------------
    @torch.no_grad()
    def retrieve_coarse_to_fine_from_feat(self, query_feat, reference_feat, all_relativeR, template_poses, stage_of=None, robust=None, **kw):
        """The retrieval in stages over a nested grid (nope_amd.search.coarse_to_fine_search, whose keyword arguments pass through): only
        the poses the search admits get a U-Net pass and a score.  Returns its C2FResult: a sparse similarity (B,N) with -inf where nothing
        was evaluated -- an ordinary input to pose_distribution and refine_from_feat -- and nearest_idx (B,k).  query_feat, reference_feat
        (B,C,h,w) f32; all_relativeR (B,N,6); template_poses (B|1,N,3,3); stage_of (N,) on the host (nope_amd.poses.grid_stages; None: the
        synthesised icosphere grid of this size, poses.grid_stages_for_size).  As with the refinement, the f16x2 range check of a stage's
        forward is not deferred: the next stage's candidates depend on its scores.  With synthetic weights the score landscape is not
        smooth: nothing is claimed about how often the search meets the exhaustive answer on real data.
        robust: as retrieval_from_feat -- every stage is scored with hip.robust_similarity, the same bits the exhaustive robust row holds."""
        from .search import coarse_to_fine_search
        if self.similarity_metric != "l2":
            return None
        if self.template_parallel and ndist.world()[1] > 1:
            raise NotImplementedError("coarse-to-fine retrieval under template_parallel with more than one rank: the stages are too small to shard")
        if stage_of is None:
            from .poses import grid_stages_for_size
            stage_of = grid_stages_for_size(all_relativeR.shape[1])
        query_feat, reference_feat = query_feat.float().contiguous(), reference_feat.float().contiguous()
        C, h, w = query_feat.shape[1:]

        def evaluate(rows, cand):
            maps = torch.empty((rows.shape[0], rows.shape[1], C, h, w), dtype=torch.float32, device=rows.device)
            return self._score(query_feat, self._forward_poses(reference_feat, rows, maps), robust)
        return coarse_to_fine_search(evaluate, all_relativeR, template_poses, stage_of, **kw)

    @torch.no_grad()
    def retrieve_coarse_to_fine(self, query, reference, all_relativeR, template_poses, stage_of=None, robust=None, **kw):
        """Encode both images, then retrieve_coarse_to_fine_from_feat (same keyword arguments)."""
        return self._encode_retrieve_coarse_to_fine(query, reference, all_relativeR, template_poses, stage_of, robust=robust, **kw)[0]

    def _encode_retrieve_coarse_to_fine(self, query, reference, all_relativeR, template_poses, stage_of=None, **kw):
        enc = self.u_net.encoder
        query_feat = enc.encode_image(query, mode="mode")
        reference_feat = enc.encode_image(reference, mode="mode")
        return self.retrieve_coarse_to_fine_from_feat(query_feat, reference_feat, all_relativeR, template_poses, stage_of, **kw), query_feat, reference_feat

    # ---- multi-reference retrieval (no reference counterpart: DESIGN.md section 4.12) ---------------------------------------------------
    def _no_multi_ref_shards(self):
        if self.template_parallel and ndist.world()[1] > 1:
            raise NotImplementedError("multi-reference retrieval under template_parallel with more than one rank: sharded banks are not fused")

    @torch.no_grad()
    def generate_templates_multi_from_feat(self, reference_feats, all_relativeR):
        """reference_feats (B,R,C,h,w), all_relativeR (B,R,N,6) -> the bank (B,R,N,C,h,w): every (sample, reference) pair is one source of
        generate_templates_from_feat -- same chunking, and the f16x2 range check is finished there."""
        self._no_multi_ref_shards()
        B, R, N = all_relativeR.shape[:3]
        if tuple(reference_feats.shape[:2]) != (B, R):
            raise hip.NopeError(f"reference_feats {tuple(reference_feats.shape)} / all_relativeR {tuple(all_relativeR.shape)}: expected (B, R, C, h, w) and (B, R, N, 6)")
        bank = self.generate_templates_from_feat(reference_feats.reshape(B * R, *reference_feats.shape[2:]).contiguous(),
                                                 all_relativeR.reshape(B * R, N, 6))
        return bank.view(B, R, N, *bank.shape[2:])

    @torch.no_grad()
    def retrieve_multi_from_feat(self, query_feat, reference_feats, ref_poses, template_poses, n_refs=None, fusion="feature", weighting="softmax",
                                 tau_deg=30.0, dist_kind=hip.C2F_ROTATION, k=5, return_per_reference=False, max_refs=None, robust=None):
        """Retrieval from R posed reference views per sample (include/nope_hip.h: nope_op_multiref_prepare, nope_multiref_similarity,
        nope_op_multiref_fuse_scores).  query_feat (B,C,h,w); reference_feats (B,R,C,h,w); ref_poses (B,R,3,3), the references' object-to-camera
        rotations in the frame of the grid; template_poses (B|1,N,3,3); n_refs (B,) or None: references r >= n_refs[b] are padding.
        fusion "feature": the U-Net's predictions from the R references are blended per grid pose and the query is scored once against the
        blend; "score": the R single-reference score rows are averaged under the same weights.  weighting "uniform" | "softmax" (over
        -distance / tau_deg between grid pose and reference pose: a reference predicts best near its own view -- a design choice, not a
        measured gain: there are no trained weights) | "nearest".  Returns a MultiRefResult; its similarity is an ordinary input to
        pose_distribution.  None for a metric the reference does not implement.
        max_refs (None: every pose is generated from all R references, B R N U-Net hypotheses): every pose is generated from its M =
        max_refs nearest references only (nope_op_multiref_select), B M N hypotheses whatever R is, and the weights -- softmax over the
        kept references -- , per_reference and the bank carry M slots in place of the R references.  M = 1 is
        "nearest" at the cost of one reference: its row is nope_similarity's, which reads no weights."""
        self._no_robust_multi(robust)
        if self.similarity_metric != "l2":
            return None
        self._no_multi_ref_shards()
        if fusion not in ("feature", "score"):
            raise ValueError(f"fusion {fusion!r}: 'feature' or 'score'")
        query_feat = query_feat.float().contiguous()
        if max_refs is not None:
            M = self._check_max_refs(max_refs, reference_feats.shape[1])
            sel = hip.op_multiref_select(template_poses, ref_poses.to(query_feat.device), n_refs, max_refs=M, weighting=weighting, tau_deg=tau_deg,
                                         dist_kind=dist_kind)
            similarity, per_ref, bank = self._score_selected(query_feat, reference_feats, sel, fusion, return_per_reference, self.bank_dtype)
            _, nearest_idx = hip.topk(similarity, k)
            return MultiRefResult(similarity, nearest_idx, sel.weights, per_ref, bank, sel.src)
        prep = hip.op_multiref_prepare(template_poses, ref_poses.to(query_feat.device), n_refs, weighting=weighting, tau_deg=tau_deg,
                                       dist_kind=dist_kind)
        bank = self.generate_templates_multi_from_feat(reference_feats, prep.all_relativeR)
        B, R, N = bank.shape[:3]
        per_ref = None
        if fusion == "score" or return_per_reference:
            per_ref = hip.similarity(query_feat, bank.view(B, R * N, *bank.shape[3:])).view(B, R, N)
        if fusion == "feature":
            similarity = hip.multiref_similarity(query_feat, bank, prep.weights)
        else:
            similarity = hip.op_multiref_fuse_scores(per_ref, prep.weights)
        _, nearest_idx = hip.topk(similarity, k)
        return MultiRefResult(similarity, nearest_idx, prep.weights, per_ref if return_per_reference else None, bank)

    # ---- the M nearest references per pose ----
    @staticmethod
    def _check_max_refs(max_refs, R):
        M = int(max_refs)
        if not 1 <= M <= R:
            raise ValueError(f"max_refs {max_refs}: 1 .. R = {R}")
        return M

    def _generate_selected(self, reference_feats, sel, out_dtype="f32"):
        """The bank (B,M,S,C,h,w) of a selection (hip.op_multiref_select): hypothesis (b, m, s) is the U-Net's map of sel.all_relativeR[b, m, s]
        from reference sel.src[b, m, s].  Every hypothesis brings its own gathered source (forward_hypotheses with one pose per source), in
        chunks of max_hypotheses_per_launch; the f16x2 range check is not deferred."""
        B, M, S = sel.src.shape
        feat = reference_feats.shape[2:]
        x = hip.op_multiref_gather(reference_feats, sel.src).view(B * M * S, *feat)
        poses = sel.all_relativeR.view(B * M * S, 1, 6)
        bank = torch.empty((B * M * S, 1, self.u_net.channels, *feat[1:]), dtype=hip.torch_dtype(hip.dtype_code(out_dtype)), device=x.device)
        for i in range(0, B * M * S, self.max_hyp):
            j = min(B * M * S, i + self.max_hyp)
            self.u_net.forward_hypotheses(x[i:j], poses[i:j], out=bank[i:j], out_dtype=out_dtype, defer_range_check=False)
        return bank.view(B, M, S, *bank.shape[2:])

    def _score_selected(self, query_feat, reference_feats, sel, fusion, want_per_ref=False, out_dtype="f32"):
        """(scores (B,S), the per-slot rows (B,M,S) or None, the bank) of a selection: the ABI 21 scoring with R := M; M = 1: nope_similarity."""
        bank = self._generate_selected(reference_feats, sel, out_dtype)
        B, M, S = bank.shape[:3]
        per_ref = None
        if M == 1:
            scores = hip.similarity(query_feat, bank.view(B, S, *bank.shape[3:]))
            return scores, (scores.view(B, 1, S) if want_per_ref else None), bank
        if fusion == "score" or want_per_ref:
            per_ref = hip.similarity(query_feat, bank.view(B, M * S, *bank.shape[3:])).view(B, M, S)
        if fusion == "feature":
            scores = hip.multiref_similarity(query_feat, bank, sel.weights)
        else:
            scores = hip.op_multiref_fuse_scores(per_ref, sel.weights)
        return scores, (per_ref if want_per_ref else None), bank

    @torch.no_grad()
    def retrieve_multi_coarse_to_fine_from_feat(self, query_feat, reference_feats, ref_poses, template_poses, n_refs=None, max_refs=1,
                                                fusion="feature", weighting="softmax", tau_deg=30.0, ref_dist_kind=hip.C2F_ROTATION,
                                                stage_of=None, robust=None, **kw):
        """retrieve_coarse_to_fine_from_feat from R posed references: every pose the search admits is generated from its max_refs nearest
        references and scored as retrieve_multi_from_feat(max_refs=...) scores it.  ref_dist_kind is the distance between grid pose and
        reference pose (retrieve_multi_from_feat's dist_kind); the search's own keyword arguments -- its dist_kind between grid poses among
        them -- pass through.  Returns the search's C2FResult."""
        from .search import coarse_to_fine_search
        self._no_robust_multi(robust)
        if self.similarity_metric != "l2":
            return None
        self._no_multi_ref_shards()
        if fusion not in ("feature", "score"):
            raise ValueError(f"fusion {fusion!r}: 'feature' or 'score'")
        M = self._check_max_refs(max_refs, reference_feats.shape[1])
        query_feat = query_feat.float().contiguous()
        ref_poses = ref_poses.to(query_feat.device)
        if stage_of is None:
            from .poses import grid_stages_for_size
            stage_of = grid_stages_for_size(template_poses.shape[1])
        B, N = query_feat.shape[0], template_poses.shape[1]
        # the search only gathers pose rows from its all_relativeR and hands them to `evaluate`, which makes its own: any finite rows do
        rows = hip.op_multiref_select(template_poses, ref_poses, n_refs, max_refs=1, weighting="nearest", dist_kind=ref_dist_kind).all_relativeR

        def evaluate(_, cand):
            sel = hip.op_multiref_select(template_poses, ref_poses, n_refs, max_refs=M, cand=cand, weighting=weighting, tau_deg=tau_deg,
                                         dist_kind=ref_dist_kind)
            return self._score_selected(query_feat, reference_feats, sel, fusion)[0]
        return coarse_to_fine_search(evaluate, rows.view(B, N, 6), template_poses, stage_of, **kw)

    @torch.no_grad()
    def refine_multi_from_feat(self, query_feat, reference_feats, ref_poses, template_poses, nearest_idx, n_refs=None, dist_kind=hip.C2F_ROTATION,
                               iters=3, fd_step=1e-2, max_step_deg=10.0, damping=1e-6):
        """refine_from_feat from R posed references: each of the k candidates nearest_idx (B,k) is refined through ITS nearest reference
        (nope_op_multiref_select with the candidates and M = 1).  The accept / revert baseline, score_init, is the score of the grid pose
        predicted from that same reference -- slot 0 of the first iteration's forward --, not the fused row's.  template_poses (B|1,N,3,3)
        is needed; pred_R does not depend on the reference.  Returns a RefineResult."""
        self._no_multi_ref_shards()
        query_feat = query_feat.float().contiguous()
        B, k = nearest_idx.shape
        sel = hip.op_multiref_select(template_poses, ref_poses.to(query_feat.device), n_refs, max_refs=1, cand=nearest_idx, weighting="nearest",
                                     dist_kind=dist_kind)
        x = hip.op_multiref_gather(reference_feats, sel.src).view(B * k, *reference_feats.shape[2:])

        def forward(poses, out):                    # candidate-major: (B, n k, 6) is (B k, n, 6), n = 7 or 1
            n = poses.shape[1] // k
            self._forward_poses(x, poses.view(B * k, n, 6), out.view(B * k, n, *out.shape[2:]))
            return out
        slot = torch.arange(k, device=query_feat.device).expand(B, k).contiguous()
        return self._refine(query_feat, forward, sel.all_relativeR.view(B, k, 6), slot, nearest_idx, None, iters, fd_step, max_step_deg, damping,
                            template_poses)

    def _encode_multi(self, query, references):
        """(query_feat, reference_feats (B,R,C,h,w)): the references encoded as one batch of B R images; the query's encoder pass runs on the
        side stream underneath them, as in generate_and_retrieve."""
        B, R = references.shape[:2]
        enc = self.u_net.encoder
        with hip.overlap_stream(query) as side:
            query_feat = enc.encode_image(query, mode="mode")
        reference_feats = enc.encode_image(references.reshape(B * R, *references.shape[2:]), mode="mode")
        side.join(query_feat)
        return query_feat, reference_feats.reshape(B, R, *reference_feats.shape[1:])

    @torch.no_grad()
    def retrieve_multi(self, query, references, reference_poses, template_poses, **kw):
        """Encode, then retrieve_multi_from_feat (same keyword arguments).  query (B,3,S,S); references (B,R,3,S,S), encoded as one batch of
        B R images; the query's encoder pass runs on the side stream underneath them, as in generate_and_retrieve."""
        if self.similarity_metric != "l2":
            return None
        self._no_multi_ref_shards()
        query_feat, reference_feats = self._encode_multi(query, references)
        return self.retrieve_multi_from_feat(query_feat, reference_feats, reference_poses, template_poses, **kw)

    @torch.no_grad()
    def retrieve_multi_coarse_to_fine(self, query, references, reference_poses, template_poses, **kw):
        """Encode, then retrieve_multi_coarse_to_fine_from_feat (same keyword arguments)."""
        if self.similarity_metric != "l2":
            return None
        self._no_multi_ref_shards()
        query_feat, reference_feats = self._encode_multi(query, references)
        return self.retrieve_multi_coarse_to_fine_from_feat(query_feat, reference_feats, reference_poses, template_poses, **kw)

    _REFINE_KEYS = ("fd_step", "max_step_deg", "damping")

    @torch.no_grad()
    def predict_pose_multi(self, query, references, reference_poses, template_poses, distinct_deg=None, symmetry=None, temperature=1.0,
                           max_refs=None, coarse_to_fine=None, refine_iters=0, robust=None, **kw):
        """predict_pose from R posed references: (pred_R (B,k,3,3) f64, score (B,k) f32) = template_poses[nearest_idx] and the fused scores of
        retrieve_multi (whose keyword arguments pass through); pred_R[:, 0] is the answer.  distinct_deg (None: the plain top-k): the k
        candidates are the seeds of the distinct modes of the fused row within that radius under `symmetry` (op_pose_modes with fill, as
        predict_pose).  max_refs (None: all R references per pose): retrieve_multi_from_feat's.  coarse_to_fine (None: the exhaustive
        retrieval; True, or a dict of the search's keyword arguments): retrieve_multi_coarse_to_fine_from_feat with max_refs (None: 1).
        refine_iters above 0: the candidates refined by refine_multi_from_feat (fd_step, max_step_deg, damping pass to it), in ITS order.
        robust: NotImplementedError unless None, as on every multi-reference method."""
        self._no_robust_multi(robust)
        if self.similarity_metric != "l2":
            return None
        self._no_multi_ref_shards()
        refine_kw = {key: kw.pop(key) for key in self._REFINE_KEYS if key in kw}
        query_feat, reference_feats = self._encode_multi(query, references)
        if coarse_to_fine is not None and coarse_to_fine is not False:
            c2f_kw = {} if coarse_to_fine is True else dict(coarse_to_fine)
            unknown = sorted(set(kw) - {"n_refs", "fusion", "weighting", "tau_deg", "k", "dist_kind"})
            if unknown:          # (the exhaustive branch raises for them as well: nothing is dropped silently)
                raise TypeError(f"predict_pose_multi(coarse_to_fine=...) got unexpected keyword arguments {unknown}")
            c2f_kw.update({("ref_dist_kind" if key == "dist_kind" else key): v for key, v in kw.items()})
            r = self.retrieve_multi_coarse_to_fine_from_feat(query_feat, reference_feats, reference_poses, template_poses,
                                                             max_refs=1 if max_refs is None else max_refs, **c2f_kw)
        else:
            r = self.retrieve_multi_from_feat(query_feat, reference_feats, reference_poses, template_poses, max_refs=max_refs, **kw)
        similarity, nearest_idx = r.similarity, r.nearest_idx
        if distinct_deg is not None:
            nearest_idx = hip.op_pose_modes(similarity, template_poses, symmetry, temperature=temperature, radius_deg=distinct_deg,
                                            max_modes=nearest_idx.shape[1], fill=True, want_prob=False).idx
        if refine_iters > 0:
            rr = self.refine_multi_from_feat(query_feat, reference_feats, reference_poses, template_poses, nearest_idx, n_refs=kw.get("n_refs"),
                                             dist_kind=kw.get("dist_kind", hip.C2F_ROTATION), iters=refine_iters, **refine_kw)
            return rr.pred_R, rr.score
        tp = template_poses.to(device=nearest_idx.device, dtype=torch.float64)
        rows = torch.arange(nearest_idx.shape[0], device=nearest_idx.device)[:, None] if tp.shape[0] != 1 else 0
        return tp[rows, nearest_idx], torch.gather(similarity, 1, nearest_idx)

    @torch.no_grad()
    def predict_pose(self, query, reference, all_relativeR, template_poses, refine_iters=0, distinct_deg=None, symmetry=None, temperature=1.0,
                     coarse_to_fine=None, robust=None, **kw):
        """(pred_R (B,k,3,3) f64, score (B,k) f32): the k best poses of the query.  refine_iters = 0: template_poses[nearest_idx]
        (model.py:352-354) and the retrieval scores; above 0: those candidates refined below the grid spacing (refine_from_feat, whose
        keyword arguments pass through), in ITS order.  template_poses (B|1,N,3,3).  None for a metric the reference does not implement.
        distinct_deg (None: the plain top-k, every output as without the argument): the k = 5 candidates are the seeds of the distinct
        modes within that radius under `symmetry` (op_pose_modes with fill: always k valid candidates), not a vertex and its neighbours.
        coarse_to_fine (None: the exhaustive retrieval, every output as without the argument; True, or a dict of
        retrieve_coarse_to_fine_from_feat's keyword arguments): the scores come from the search in stages over the nested grid instead --
        a sparse row, -inf where nothing was evaluated, on which distinct_deg and refine_iters work unchanged.
        robust (None: every output as without the argument): as retrieval_from_feat; the exhaustive row or every stage of the search is
        the robust score.  With refine_iters > 0 it raises NotImplementedError: the refinement's cost and its accept / revert are defined
        on the plain metric."""
        if robust is not None and refine_iters > 0:
            raise NotImplementedError("robust scoring with refine_iters > 0: the refinement's cost and its accept / revert are defined on the plain metric")
        if self.similarity_metric != "l2":
            return None
        if coarse_to_fine is not None and coarse_to_fine is not False:
            c2f_kw = {} if coarse_to_fine is True else dict(coarse_to_fine)
            if robust is not None:
                c2f_kw["robust"] = robust
            c2f, query_feat, reference_feat = self._encode_retrieve_coarse_to_fine(query, reference, all_relativeR, template_poses, **c2f_kw)
            similarity, nearest_idx = c2f.similarity, c2f.nearest_idx
        else:
            similarity, nearest_idx, _, query_feat, reference_feat = self._encode_generate_retrieve(query, reference, all_relativeR, robust=robust)
        if distinct_deg is not None:
            nearest_idx = hip.op_pose_modes(similarity, template_poses, symmetry, temperature=temperature, radius_deg=distinct_deg,
                                            max_modes=nearest_idx.shape[1], fill=True, want_prob=False).idx
        if refine_iters <= 0:
            tp = template_poses.to(device=nearest_idx.device, dtype=torch.float64)
            rows = torch.arange(nearest_idx.shape[0], device=nearest_idx.device)[:, None] if tp.shape[0] != 1 else 0
            return tp[rows, nearest_idx], torch.gather(similarity, 1, nearest_idx)
        r = self.refine_from_feat(query_feat, reference_feat, all_relativeR, nearest_idx, similarity, iters=refine_iters,
                                  template_poses=template_poses, **kw)
        return r.pred_R, r.score

    # ---- evaluation, model.py:268-565 --------------------------------------------------------------------------------------------------
    def load_mesh(self, cad_dir, obj_ids=range(1, 31)):
        """obj_000001.ply ... obj_000030.ply of cad_dir into one device mesh bank (model.py:378-389), read without trimesh."""
        from . import vsd
        self.tless_cad = vsd.load_mesh_bank(cad_dir, obj_ids, device=next(self.parameters()).device)
        return self.tless_cad

    @torch.no_grad()
    def eval_vsd(self, batch, data_name, save_path=None):
        """The T-LESS evaluation (model.py:391-541) without visualisation or logging.  Returns {f"loss/val_{data_name}": the training loss
        under the ground-truth pose, and the six `final_scores` of model.py:530-537}; saves vsd_error[:, 0] to save_path (np.save) if given.
        batch: query, reference (B,3,S,S); gt_relativeR (B,6); all_relativeR (B,N,6); template_poses (B,N,3,3); query_pose (B,3,3);
        query_translation (B,3,1) mm; intrinsic (B,3,3); obj_id (B,); and depth (B,H,W) mm, or depth_path (B PNG paths, read with
        nope_amd.vsd.load_depth).  Predictions are template_poses[b, nearest_idx[b]] with the ground-truth translation (model.py:470-500);
        errors by nope_amd.vsd.vsd_error with the reference's defaults (delta 15, tau 20, step cost, bop19)."""
        import numpy as np
        from . import vsd
        if getattr(self, "tless_cad", None) is None:
            raise RuntimeError("eval_vsd: no meshes: call load_mesh(cad_dir) first (model.py:378)")
        query, reference = batch["query"], batch["reference"]
        loss = self.forward(query=query, relativeR=batch["gt_relativeR"], reference=reference)
        pred_feat, _, _ = self.generate_templates(reference=reference, all_relativeR=batch["all_relativeR"])
        out = self.retrieval(query=query, template_feat=pred_feat)
        if out is None:
            raise NotImplementedError(f"eval_vsd: similarity_metric {self.similarity_metric!r} (the reference implements 'l2' only)")
        _, nearest_idx = out
        B = query.shape[0]
        template_poses = batch["template_poses"]
        rows = torch.arange(B, device=template_poses.device)[:, None].expand(-1, nearest_idx.shape[1])
        retrieved_R = template_poses[rows, nearest_idx.to(template_poses.device)]
        if "depth" in batch:
            depth_test = batch["depth"]
        else:
            depth_test = np.stack([vsd.load_depth(p) for p in batch["depth_path"]])
        err = vsd.vsd_error(depth_test, self.tless_cad, batch["obj_id"], retrieved_R, batch["query_pose"], batch["query_translation"],
                            batch["intrinsic"])
        scores = {f"loss/val_{data_name}": float(loss)}
        scores.update(vsd.vsd_scores(err))
        if save_path is not None:
            np.save(save_path, err[:, 0].cpu().numpy())
        return scores

    def load_models_info(self, cad_dir_or_file, max_sym_disc_step=0.01):
        """models_info.json of a BOP models directory (or the file itself): the objects' diameters and symmetry sets for eval_bop
        (nope_amd.bop.load_models_info, SymmetryBank.from_models_info).  No reference counterpart: the reference reads the file
        (dataloader/baseBOP.py:284) and does not use it."""
        from . import bop
        self.tless_models_info = bop.load_models_info(cad_dir_or_file)
        self.tless_symmetries = bop.SymmetryBank.from_models_info(self.tless_models_info, device=next(self.parameters()).device,
                                                                  max_sym_disc_step=max_sym_disc_step)
        return self.tless_models_info

    @torch.no_grad()
    def eval_bop(self, batch, data_name, save_path=None, translation="gt", depth_tau=None):
        """The T-LESS evaluation under the BOP benchmark's errors: eval_vsd's batch, forward pass and retrieval, then MSSD, MSPD, ADD and
        ADI of the retrieved rotations (nope_amd.bop.pose_errors; `translation` below) and VSD over tau in 0.05 ... 0.50 times the
        diameter (delta 15, step cost, bop19) from ONE rendering.  Returns {f"loss/val_{data_name}", and nope_amd.bop.bop_scores' recalls:
        AR_MSSD, AR_MSPD, AR_VSD, AR, ADD / ADD-S at 0.1 d, for the top 1 / 3 / 5}.  Symmetries and diameters come from load_models_info;
        without it the symmetry sets are the identity and the diameters are measured on the meshes (bop.mesh_diameters).  save_path:
        np.savez of the error tables.  No reference counterpart (eval_vsd is the reference's evaluation); nothing is claimed about
        accuracy on real data.
        translation: "gt" -- the estimates take the ground-truth translation (the rotation retriever alone is measured);
        "box" -- each of the k rotations gets the translation that fits the detection, batch["box"] (B, 4) = (u0, v0, u1, v1) or
        batch["mask"] (B, H, W) (bop.estimate_translation): a 6D pose of the library's own; "box+depth" -- and its distance is corrected
        on batch["depth"] within depth_tau mm (bop.refine_translation_depth, inliers inside batch["mask"] if there is one).  A candidate
        whose translation status is not 0 is a miss: +inf in every error table.  The saved tables then hold t, residual and status too."""
        import numpy as np
        from . import bop, vsd
        if getattr(self, "tless_cad", None) is None:
            raise RuntimeError("eval_bop: no meshes: call load_mesh(cad_dir) first (model.py:378)")
        if translation not in ("gt", "box", "box+depth"):
            raise ValueError(f"eval_bop: translation {translation!r} (known: 'gt', 'box', 'box+depth')")
        if translation != "gt" and batch.get("box") is None and batch.get("mask") is None:
            raise ValueError(f"eval_bop: translation={translation!r} needs the detection: batch['box'] (B, 4) or batch['mask'] (B, H, W)")
        if translation == "box+depth" and depth_tau is None:
            raise ValueError("eval_bop: translation='box+depth' needs depth_tau (mm): nothing here is tuned")
        query, reference = batch["query"], batch["reference"]
        loss = self.forward(query=query, relativeR=batch["gt_relativeR"], reference=reference)
        pred_feat, _, _ = self.generate_templates(reference=reference, all_relativeR=batch["all_relativeR"])
        out = self.retrieval(query=query, template_feat=pred_feat)
        if out is None:
            raise NotImplementedError(f"eval_bop: similarity_metric {self.similarity_metric!r} (the reference implements 'l2' only)")
        _, nearest_idx = out
        B = query.shape[0]
        template_poses = batch["template_poses"]
        rows = torch.arange(B, device=template_poses.device)[:, None].expand(-1, nearest_idx.shape[1])
        retrieved_R = template_poses[rows, nearest_idx.to(template_poses.device)]
        if "depth" in batch:
            depth_test = batch["depth"]
        else:
            depth_test = np.stack([vsd.load_depth(p) for p in batch["depth_path"]])
        obj_ids = [int(o) for o in (batch["obj_id"].tolist() if hasattr(batch["obj_id"], "tolist") else batch["obj_id"])]
        info = getattr(self, "tless_models_info", None)
        if info is not None and all(o in info and "diameter" in info[o] for o in obj_ids):
            diam = np.array([float(info[o]["diameter"]) for o in obj_ids])
        else:
            if getattr(self, "_tless_diameters", None) is None or self._tless_diameters[0] is not self.tless_cad:
                self._tless_diameters = (self.tless_cad, bop.mesh_diameters(self.tless_cad))
            diam = np.array([self._tless_diameters[1][o] for o in obj_ids])
        pred_t = fit = miss = None
        if translation != "gt":
            cad_dev = self.tless_cad.device
            if batch.get("box") is not None:
                fit = bop.estimate_translation(self.tless_cad, obj_ids, retrieved_R, batch["intrinsic"], box=batch["box"])
            else:
                fit = bop.estimate_translation(self.tless_cad, obj_ids, retrieved_R, batch["intrinsic"], mask=batch["mask"])
            status = fit["status"]
            gt_t = vsd._as_f64(batch["query_translation"], cad_dev).reshape(B, 1, 3)
            # a candidate without a usable translation is a miss below; it is rendered at the ground truth's, which can be rendered
            pred_t = torch.where((status != 0)[..., None], gt_t, fit["t"])
            if translation == "box+depth":
                dep = bop.refine_translation_depth(self.tless_cad, obj_ids, retrieved_R, pred_t, batch["intrinsic"], depth_test, depth_tau,
                                                   mask=batch.get("mask"))
                status = status | dep["status"]
                pred_t = torch.where((status != 0)[..., None], gt_t, dep["t"])
            fit = dict(fit, t=torch.where((status != 0)[..., None], fit["t"], pred_t), status=status)
            miss = status != 0
        errors = bop.pose_errors(self.tless_cad, getattr(self, "tless_symmetries", None), obj_ids, retrieved_R, batch["query_pose"],
                                 batch["query_translation"], batch["intrinsic"], pred_t=pred_t)
        _, d_gt, d_est = vsd.vsd_error(depth_test, self.tless_cad, obj_ids, retrieved_R, batch["query_pose"], batch["query_translation"],
                                       batch["intrinsic"], return_depth=True, pred_t=pred_t)
        dev = d_est.device
        dtest = (depth_test if isinstance(depth_test, torch.Tensor) else torch.from_numpy(np.asarray(depth_test))).to(dev)
        # tau differs per query (a fraction of its object's diameter): queries of one diameter share a launch
        vsd_stack = torch.empty((len(bop.THRESHOLDS),) + tuple(d_est.shape[:2]), dtype=torch.float64, device=dev)
        Kt = vsd._as_f64(batch["intrinsic"], dev)
        if Kt.dim() == 2:
            Kt = Kt.reshape(1, 3, 3).expand(B, 3, 3)
        for d in sorted(set(diam.tolist())):
            sel = torch.from_numpy(np.nonzero(diam == d)[0]).to(dev)
            for ti, frac in enumerate(bop.THRESHOLDS):
                vsd_stack[ti, sel] = vsd.vsd_from_depth(dtest[sel], d_gt[sel].contiguous(), d_est[sel].contiguous(), Kt[sel].contiguous(),
                                                        delta=15, tau=frac * d)
        extra = {}
        if miss is not None:
            inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
            errors = {m: (torch.where(miss.to(e.device), inf.to(e.device), e) if m in bop.METRICS else e) for m, e in errors.items()}
            vsd_stack = torch.where(miss.to(dev)[None], inf, vsd_stack)
            extra = {name: fit[name].cpu().numpy() for name in ("t", "residual", "status")}
        width = depth_test.shape[-1]
        scores = {f"loss/val_{data_name}": float(loss)}
        scores.update(bop.bop_scores(errors, diam, width, vsd_errors=vsd_stack))
        if save_path is not None:
            np.savez(save_path, vsd=vsd_stack.cpu().numpy(), diameter=diam, **{m: errors[m].cpu().numpy() for m in bop.METRICS}, **extra)
        return scores

    @torch.no_grad()
    def eval_geodesic(self, batch, data_name, visualize=False, save_prediction=False):
        """model.py:268-376 through nope_amd.harness.eval_geodesic: {"loss", geodesic / accuracy scores}.  save_prediction writes
        predictions/pred_step{global_step}_rank{global_rank}.npz (with save_dir).  visualize (with a decoding encoder and save_dir; forced
        off otherwise, model.py:269-274) writes media/reconst_step*.png, the template pictures and video of generate_templates and
        media/retrieved_step*.png, and adds `vis_imgs` to the npz; scores, indices and metrics are those of visualize=False."""
        from .harness import eval_geodesic
        save = None
        if save_prediction and self.save_dir is not None:
            save = os.path.join(self.save_dir, "predictions", f"pred_step{self.global_step}_rank{self.global_rank}")
        _, _, res = eval_geodesic(self, batch, save_path=save, visualize=visualize)
        return res

    def validation_step(self, batch, idx):
        """model.py:543-548: "tless" -> eval_vsd, every other dataloader -> eval_geodesic.  Returns {data_name: scores}."""
        out = {}
        for data_name in batch.keys():
            if data_name in ["tless"]:
                out[data_name] = self.eval_vsd(batch[data_name], data_name)
            else:
                out[data_name] = self.eval_geodesic(batch[data_name], data_name)
        return out

    def test_step(self, batch, idx_batch):
        """model.py:550-565: dataloaders keyed "<data>_<category>"; tless -> eval_vsd (errors saved to
        predictions/vsd_{category}_batch{idx_batch}_rank_{global_rank}.npy with save_dir), otherwise eval_geodesic with saved predictions.
        Returns {dataloader_name: scores}."""
        out = {}
        for dataloader_name in batch.keys():
            data_name, category = dataloader_name.split("_", 1)
            if data_name in ["tless"]:
                save_path = None
                if self.save_dir is not None:
                    save_path = os.path.join(self.log_dir, f"vsd_{category}_batch{idx_batch}_rank_{self.global_rank}.npy")
                out[dataloader_name] = self.eval_vsd(batch[dataloader_name], category, save_path=save_path)
            else:
                out[dataloader_name] = self.eval_geodesic(batch[dataloader_name], category, visualize=True, save_prediction=True)
        return out
