"""Tuning aid: the guided-diffusion variant at its shipped size (configs/model/vae_guidedDiffusion.yaml: 552.8 M parameters), a batch of
pose hypotheses at a 32x32 latent (run under rocprofv3 --kernel-trace --stats for the per-kernel split; prints hypotheses/s and the
fraction of the dense peak the forward reaches at 34.9 GFLOP per hypothesis).

    python tools/guided_step.py [N] [--dtype bf16|f16|f32|bf16x3|f16x2]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from nope_amd.guided import UNetModelPose
from nope_amd.weights import synth_init_
from tests.util import StubEncoder

GFLOP_PER_HYP = 34.9
PEAK_TFLOPS = {"f32": 157.3, "bf16x3": 2516.6 / 3, "f16x2": 2516.6 / 2, "bf16": 2516.6, "f16": 2516.6}   # MI355X dense MFMA peak per mode's pass count


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 128
    dtype = sys.argv[sys.argv.index("--dtype") + 1] if "--dtype" in sys.argv else "bf16"
    kw = dict(pose_mlp_name="single_layer", rot_representation_dim=6, image_size=256, in_channels=4, model_channels=256, out_channels=4,
              num_res_blocks=2, attention_resolutions=[32, 16, 8], channel_mult=(1, 1, 2, 2, 4, 4), num_head_channels=64, num_heads=4,
              num_heads_upsample=-1, resblock_updown=True, use_scale_shift_norm=True)
    m = UNetModelPose(encoder=StubEncoder(4), compute_dtype=dtype, **kw)
    synth_init_(m, 2022)
    m = m.cuda()
    g = torch.Generator().manual_seed(3)
    x, poses = torch.randn(1, 4, 32, 32, generator=g).cuda(), torch.randn(1, n, 6, generator=g).cuda()
    m.forward_hypotheses(x, poses)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        m.forward_hypotheses(x, poses)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    tflops = n * GFLOP_PER_HYP / dt / 1e3
    print(f"guided {dtype}, {n} hypotheses at 32x32: {dt * 1e3:.1f} ms per forward = {n / dt:.0f} hypotheses/s = {tflops:.0f} TFLOP/s "
          f"({tflops / PEAK_TFLOPS[dtype]:.2f} of the {PEAK_TFLOPS[dtype]:.0f} TFLOP/s dense peak of the mode's MFMA passes)")


if __name__ == "__main__":
    main()
