"""Terrain estimator timings -> profiles/terrain_estimator.json: the depth encoder alone and the whole estimator step, native
(`lg_conv_encoder_forward` / `lg_estimator_step`) against the eager fp32 torch module of `tools/train_estimator.py` on the same card (MIOpen
convolutions: what a user would run otherwise).  4096 envs, 28 x 56, default widths, HIP events, warm, interleaved in one process in the order
native / eager / native / eager; the median of the per-block means is reported with the spread of the blocks.  Also the encoder's fraction of
the fp32 matrix peak (157 TFLOP/s, the figure profiles/r06_f_other_kernels.json uses for PPO.act), from the multiply-add count recomputed
from the layer shapes.  The depth-camera update the estimator consumes is timed by `tools/bench_configs.py 4`.

    python tools/bench_estimator.py [--envs 4096] [--out profiles/terrain_estimator.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PEAK_F32_MATRIX_TFLOPS = 157.0


def encoder_macs(height, width, out_dim=64):
    """Multiply-adds of the encoder per image, from the layer shapes."""
    total, h, w, per = 0, height, width, {}
    for name, (cin, cout, k, s, p) in zip(("conv1", "conv2", "conv3", "conv4"), ((1, 32, 5, 2, 2), (32, 64, 3, 2, 1), (64, 128, 3, 2, 1), (128, 64, 3, 1, 1))):
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        per[name] = h * w * cout * cin * k * k
    per["linear1"], per["linear2"] = 1024 * 128, 128 * out_dim
    total = sum(per.values())
    return total, per


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terrain_estimator.json"))
    a = ap.parse_args(argv)
    from extended_legged_gym_amd.rl import NativeTerrainEstimator
    from train_estimator import TerrainEstimatorTorch
    n, shape, P, R = a.envs, (28, 56), 6, 512
    torch.manual_seed(0)
    eager = TerrainEstimatorTorch(shape, P, R).cuda().eval()
    native = NativeTerrainEstimator({k: v.detach().cpu() for k, v in eager.state_dict().items()}, shape, P, device="cuda:0")
    fifo = torch.rand(n, 2, *shape, device="cuda")
    proprio = torch.randn(n, P, device="cuda")
    cases = {
        "encoder_native": lambda: native.encoder(fifo),
        "encoder_eager": lambda: eager.encode(fifo),
        "step_native": lambda: native.act_inference(fifo, proprio),
        "step_eager": lambda: eager.act_inference(fifo, proprio),
    }
    with torch.inference_mode():
        for fn in cases.values():                       # warm: MIOpen picks its kernels, the workspaces are allocated
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        blocks = {k: [] for k in cases}
        for _ in range(a.blocks):
            for pair in (("encoder_native", "encoder_eager"), ("step_native", "step_eager")):
                for _ in range(2):                      # native / eager / native / eager
                    for k in pair:
                        blocks[k].append(timed(cases[k], a.iters))
        err = float((native.encoder(fifo) - eager.encode(fifo)).abs().max())
    macs, per = encoder_macs(*shape)
    res = {k + "_ms": float(np.median(v)) for k, v in blocks.items()}
    res.update({k + "_ms_min_max": [float(min(v)), float(max(v))] for k, v in blocks.items()})
    tflops = 2.0 * macs * n / (res["encoder_native_ms"] * 1e-3) / 1e12
    lib = os.path.join(ROOT, "extended_legged_gym_amd", "csrc", "liblgstep.so")
    res.update(envs=n, image=list(shape), raycast_outputs=R, iters_per_block=a.iters, blocks_per_case=2 * a.blocks,
               encoder_macs_per_env=macs, encoder_macs_per_layer=per, encoder_tflops=tflops, peak_f32_matrix_tflops=PEAK_F32_MATRIX_TFLOPS,
               encoder_fraction_of_peak=tflops / PEAK_F32_MATRIX_TFLOPS, native_vs_eager_encoder_max_abs_diff=err,
               step_native_not_slower_than_eager=res["step_native_ms"] <= res["step_eager_ms"],
               device=torch.cuda.get_device_name(0), torch=torch.__version__, date=time.strftime("%Y-%m-%d"),
               library_sha256=subprocess.run(["sha256sum", lib], capture_output=True, text=True).stdout.split()[0][:16])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
