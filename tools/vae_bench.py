"""Times of the Stable Diffusion VAE on the device (SD-1.5 shapes, synthetic weights): encode of one 256^2 image and decode of a batch of
256^2 images per compute mode, the one-head attention at 1 024 tokens, and the decoder's top-level 3x3 convs as a fraction of the dense
peak.  One JSON line per measurement.

    python tools/vae_bench.py [--modes f32,bf16x3,f16,bf16] [--decode-batch 32] [--reps 5]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nope_amd import hip  # noqa: E402
from nope_amd.vae import SD15_CONFIG, VAE_StableDiffusion  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="f32,bf16x3,f16,bf16")
    ap.add_argument("--decode-batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    img = (torch.rand(1, 3, 256, 256, generator=g) * 2 - 1).cuda()
    lat = torch.randn(a.decode_batch, 4, 32, 32, generator=g).cuda()
    for mode in a.modes.split(","):
        vae = VAE_StableDiffusion(None, config=SD15_CONFIG, compute_dtype=mode).synth_init_(2023).cuda()
        enc_ms = timed(lambda: vae.encode_image(img), a.reps)
        dec_ms = timed(lambda: vae.decode_latent(lat), max(1, a.reps // 2))
        print(json.dumps(dict(what="vae", mode=mode, encode_ms_1x256=enc_ms, decode_ms_per_image=dec_ms / a.decode_batch,
                              decode_batch=a.decode_batch)), flush=True)
        del vae
        torch.cuda.empty_cache()
    for dt, name in ((0, "f32"), (3, "bf16x3"), (1, "bf16"), (2, "f16")):
        qkv = torch.randn(1, 1024, 3 * 512, generator=g).to(hip.torch_dtype(hip.storage_code(dt))).cuda()
        ms = timed(lambda: hip.op_wide_attention(dt, qkv), 10)
        print(json.dumps(dict(what="wide_attention", mode=name, C=512, tokens=1024, ms=ms, gflops=4 * 1024 * 1024 * 512 / ms / 1e6)), flush=True)
    # the decoder's 256^2-level 3x3 convs (128 -> 128 channels) alone, bf16, batch of 8
    for dt, name in ((1, "bf16"), (2, "f16"), (3, "bf16x3"), (0, "f32")):
        x = hip.to_nhwc(torch.randn(8, 128, 256, 256, generator=g).cuda(), dt)
        w = (torch.randn(128, 128, 3, 3, generator=g) * 0.03).cuda()
        pw, cin, ntaps = hip.pack_conv_weight(w, dt)
        out = torch.empty((8, 256, 256, 128), dtype=hip.torch_dtype(dt), device="cuda")
        l = hip.lib()

        op = ctypes.byref(hip._op_struct(hip.ConvOp, dict(dtype=dt, src1=x, C1=128, Hs=256, Ws=256, mode=hip.CONV_PLAIN, ntaps=9, w_packed=pw, out=out,
                                                          Cout=128, n_hyp=8)))

        def run():
            l.check(l.dll.nope_op_conv(op, None, hip._stream(x)), "conv")
        ms = timed(run, 10)
        tflops = 2 * 8 * 256 * 256 * 128 * 128 * 9 / ms / 1e9
        print(json.dumps(dict(what="decoder_conv3x3_256x256_128ch", mode=name, batch=8, ms=ms, tflops=tflops)), flush=True)


if __name__ == "__main__":
    main()
