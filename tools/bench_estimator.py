"""Terrain estimator timings -> profiles/terrain_estimator.json: the depth encoder alone and the whole estimator step, native
(`lg_conv_encoder_forward` / `lg_estimator_step`) against the eager fp32 torch module of `tools/train_estimator.py` on the same card (MIOpen
convolutions: what a user would run otherwise).  4096 envs, 28 x 56, default widths, HIP events, warm, interleaved in one process in the order
native / eager / native / eager; the median of the per-block means is reported with the spread of the blocks.  Also the encoder's fraction of
the fp32 matrix peak (157 TFLOP/s, the figure profiles/r06_f_other_kernels.json uses for PPO.act), from the multiply-add count recomputed
from the layer shapes.  The depth-camera update the estimator consumes is timed by `tools/bench_configs.py 4`.

`--precision bf16` times the bf16 encoder mode (`NativeTerrainEstimator(..., encoder_precision="bf16")`) under the keys `encoder_bf16*` / `step_bf16*`
instead of the fp32 native ones; `--precision both` times fp32 and bf16 back to back in the same process, interleaved per block in the order
fp32 / bf16 / fp32 / bf16, and adds their ratio, the bf16 encoder's fraction of the bf16 matrix peak (2500 TFLOP/s dense) and its map traffic
(bytes every stage must read and write once, from the layer shapes) against the time.  The fp32 keys keep their names and meaning.

    python tools/bench_estimator.py [--envs 4096] [--precision fp32|bf16|both] [--out profiles/terrain_estimator.json]
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
PEAK_BF16_MATRIX_TFLOPS = 2500.0          # MI355X dense bf16 matrix peak, 16 x the fp32 matrix figure above


def encoder_macs(height, width, out_dim=64):
    """Multiply-adds of the encoder per image, from the layer shapes."""
    total, h, w, per = 0, height, width, {}
    for name, (cin, cout, k, s, p) in zip(("conv1", "conv2", "conv3", "conv4"), ((1, 32, 5, 2, 2), (32, 64, 3, 2, 1), (64, 128, 3, 2, 1), (128, 64, 3, 1, 1))):
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        per[name] = h * w * cout * cin * k * k
    per["linear1"], per["linear2"] = 1024 * 128, 128 * out_dim
    total = sum(per.values())
    return total, per


def bf16_map_bytes(height, width, out_dim=64):
    """Bytes per image the bf16 encoder cannot avoid moving through its workspaces: every stage's map written once and read once (bf16), the fp32
    image read once and the fp32 features written once; weights not counted (shared by all images)."""
    h, w, maps = height, width, []
    for cout, k, s, p in ((32, 5, 2, 2), (64, 3, 2, 1), (128, 3, 2, 1), (64, 3, 1, 1)):
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        maps.append(h * w * cout)
    maps += [1024, 128]
    return 2 * 2 * sum(maps) + 4 * height * width + 4 * out_dim


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
    ap.add_argument("--precision", choices=("fp32", "bf16", "both"), default="fp32", help="encoder mode(s) of the native estimator to time")
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
    pairs = [("encoder_native", "encoder_eager"), ("step_native", "step_eager")]
    if a.precision != "fp32":
        low = NativeTerrainEstimator({k: v.detach().cpu() for k, v in eager.state_dict().items()}, shape, P, device="cuda:0", encoder_precision="bf16")
        cases.update(encoder_bf16=lambda: low.encoder(fifo), step_bf16=lambda: low.act_inference(fifo, proprio))
        if a.precision == "bf16":          # the bf16 mode in place of the fp32 native one
            del cases["encoder_native"], cases["step_native"]
            pairs = [("encoder_bf16", "encoder_eager"), ("step_bf16", "step_eager")]
        else:                              # fp32 / bf16 / fp32 / bf16 in the same blocks, behind the native / eager ones
            pairs += [("encoder_native_vs_bf16", "encoder_bf16"), ("step_native_vs_bf16", "step_bf16")]
            cases.update(encoder_native_vs_bf16=cases["encoder_native"], step_native_vs_bf16=cases["step_native"])
    with torch.inference_mode():
        for fn in cases.values():                       # warm: MIOpen picks its kernels, the workspaces are allocated
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        blocks = {k: [] for k in cases}
        for _ in range(a.blocks):
            for pair in pairs:
                for _ in range(2):                      # native / eager / native / eager
                    for k in pair:
                        blocks[k].append(timed(cases[k], a.iters))
        err = float((native.encoder(fifo) - eager.encode(fifo)).abs().max())          # also keeps the comparison in the default run
        err_bf16 = float((low.encoder(fifo) - eager.encode(fifo)).abs().max()) if a.precision != "fp32" else None
    macs, per = encoder_macs(*shape)
    res = {k + "_ms": float(np.median(v)) for k, v in blocks.items()}
    res.update({k + "_ms_min_max": [float(min(v)), float(max(v))] for k, v in blocks.items()})
    if a.precision != "fp32":
        tf16, traffic = 2.0 * macs * n / (res["encoder_bf16_ms"] * 1e-3) / 1e12, bf16_map_bytes(*shape)
        res.update(encoder_bf16_tflops=tf16, peak_bf16_matrix_tflops=PEAK_BF16_MATRIX_TFLOPS, encoder_bf16_fraction_of_peak=tf16 / PEAK_BF16_MATRIX_TFLOPS,
                   encoder_bf16_min_bytes_per_env=traffic, encoder_bf16_min_traffic_gb_per_s=traffic * n / (res["encoder_bf16_ms"] * 1e-3) / 1e9,
                   bf16_vs_eager_encoder_max_abs_diff=err_bf16)
    if a.precision == "both":
        for part in ("encoder", "step"):
            f32, b16 = blocks[part + "_native_vs_bf16"], blocks[part + "_bf16"]
            res[part + "_bf16_speedup_over_fp32"] = res[part + "_native_vs_bf16_ms"] / res[part + "_bf16_ms"]
            res[part + "_block_spread_ms"] = max(max(f32) - min(f32), max(b16) - min(b16))
            res[part + "_bf16_faster_by_more_than_the_spread"] = bool(min(f32) - max(b16) > res[part + "_block_spread_ms"])
    lib = os.path.join(ROOT, "extended_legged_gym_amd", "csrc", "liblgstep.so")
    if a.precision != "bf16":
        tflops = 2.0 * macs * n / (res["encoder_native_ms"] * 1e-3) / 1e12
        res.update(encoder_tflops=tflops, peak_f32_matrix_tflops=PEAK_F32_MATRIX_TFLOPS, encoder_fraction_of_peak=tflops / PEAK_F32_MATRIX_TFLOPS,
                   native_vs_eager_encoder_max_abs_diff=err, step_native_not_slower_than_eager=res["step_native_ms"] <= res["step_eager_ms"])
    res.update(envs=n, image=list(shape), raycast_outputs=R, iters_per_block=a.iters, blocks_per_case=2 * a.blocks, precision=a.precision,
               encoder_macs_per_env=macs, encoder_macs_per_layer=per,
               device=torch.cuda.get_device_name(0), torch=torch.__version__, date=time.strftime("%Y-%m-%d"),
               library_sha256=subprocess.run(["sha256sum", lib], capture_output=True, text=True).stdout.split()[0][:16])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
