"""Native terrain-estimator update (rl.NativeEstimatorDistillation, include/lgestimator_train.h) against eager torch (`estimator_update` of
tools/train_estimator.py on a `TerrainEstimatorTorch`: MIOpen's convolution backward, `nn.GRU`, autograd, `optim.Adam`) on the same rows
and the same device, interleaved in one process, by the method of tools/bench_ppo_update.py.

Shape: the registered estimator -- 4096 envs x 24 steps, 28 x 56 images, 6 base velocities, encoder 64, GRU 256 x 1, decoder 128-64, 81 rays,
gradient_length 15, one epoch: one optimiser step on 15 x 4096 rows and nine forward-only steps per update.  The rows are recorded once (closed-form
images, seeded velocities and targets) and both sides read the same tensors.  Per side: warm-up updates, then `--reps` timed updates, the sides
alternating; HIP events around each update.  Records ms per update (median, min, max) for both, the native workspace bytes, the date and the
library's hash.

The per-phase split comes from a kernel-trace run of its own (never from the timed run):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_estimator_update.py --native-only --reps 2
    python tools/bench_estimator_update.py --merge-trace DIR
which adds to the JSON the share of the traced kernel time spent in: encoder forward, conv data gradient, conv weight gradient (its slab
reduction counts under the rest), memory, the rest.

usage: python tools/bench_estimator_update.py [--reps 5] [--out profiles/estimator_update.json]"""
import argparse
import csv
import datetime
import glob
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PHASES = (("encoder_forward", ("conv_gemm_kernel", "pool_flatten_kernel", "cat_columns_kernel")),
          ("conv_data_gradient", ("est_dgrad_kernel", "est_pool_backward_kernel")),
          ("conv_weight_gradient", ("est_conv_wgrad_kernel",)),
          ("memory", ("rnn_train_forward_kernel", "rnn_backward_kernel", "rnn_retile_kernel")))


def merge_trace(directory, out):
    total, split, top = 0.0, {name: 0.0 for name, _ in PHASES}, {}
    split["rest"] = 0.0
    for f in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                ns, kernel = float(row["TotalDurationNs"]), row["Name"]
                phase = next((name for name, parts in PHASES if any(p in kernel for p in parts)), "rest")
                split[phase] += ns
                total += ns
                top[kernel.split("(")[0][:60]] = top.get(kernel.split("(")[0][:60], 0.0) + ns
    if total == 0:
        raise SystemExit(f"no kernel statistics under {directory}")
    with open(out) as f:
        doc = json.load(f)
    doc["native_phase_share"] = {k: v / total for k, v in split.items()}
    doc["native_phase_source"] = "rocprofv3 --kernel-trace --stats, a run of its own (--native-only --reps 2, warm-up included)"
    doc["native_top_kernels_share"] = {k: v / total for k, v in sorted(top.items(), key=lambda kv: -kv[1])[:8]}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["native_phase_share"]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--native-only", action="store_true", help="no torch side and no file: the run a kernel trace wraps")
    ap.add_argument("--merge-trace", default=None, help="directory of a rocprofv3 --kernel-trace --stats run: add the per-phase split to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimator_update.json"))
    a = ap.parse_args(argv)
    if a.merge_trace:
        return merge_trace(a.merge_trace, a.out)
    import torch
    from train_estimator import TerrainEstimatorTorch, closed_form_depth, closed_form_state, estimator_update
    from extended_legged_gym_amd.native import load_library
    from extended_legged_gym_amd.rl import NativeEstimatorDistillation, NativeTerrainEstimator
    T, N, shape, P, R, G, lr = 24, a.envs, (28, 56), 6, 81, 15, 1e-3
    model = TerrainEstimatorTorch(shape, P, R)
    model.load_state_dict(closed_form_state(model))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.cuda()
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    est = NativeTerrainEstimator(sd, shape, P, device="cuda:0")
    trainer = NativeEstimatorDistillation(est, sd, gradient_length=G, learning_rate=lr)
    g = torch.Generator().manual_seed(1)
    rows = dict(depth_images=closed_form_depth(T, N, *shape).cuda(), proprio_data=torch.randn(T, N, P, generator=g).cuda(),
                raycast_targets=(2.0 + torch.rand(T, N, R, generator=g)).cuda(), dones=torch.zeros(T, N).cuda())
    times, losses, hidden = {"native": [], "torch": []}, {"native": [], "torch": []}, None
    for rep in range(a.warmup + a.reps):
        for side in ("native",) if a.native_only else ("native", "torch"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            if side == "native":
                loss = trainer.update(rows)["estimation"]
            else:
                loss, hidden = estimator_update(model, opt, rows, hidden, G)
            e1.record()
            torch.cuda.synchronize()
            losses[side].append(loss)
            if rep >= a.warmup:
                times[side].append(e0.elapsed_time(e1))
    row = dict(shape="registered_28x56", envs=N, steps=T, image=list(shape), rays=R, memory="gru", memory_hidden=256, decoder=[128, 64], gradient_length=G, epochs=1,
               rows_per_group=G * N, native_workspace_bytes=trainer.workspace_bytes(), losses=losses)
    for side, ts in times.items():
        if ts:
            row[side] = dict(ms_per_update_median=statistics.median(ts), ms_per_update_min=min(ts), ms_per_update_max=max(ts), reps=len(ts))
    print(json.dumps({k: v for k, v in row.items() if k != "losses"}), flush=True)
    if a.native_only:
        return
    row["native_over_torch"] = row["native"]["ms_per_update_median"] / row["torch"]["ms_per_update_median"]
    print("native / torch:", row["native_over_torch"], flush=True)
    lib = load_library()
    digest = hashlib.sha256(open(lib._name, "rb").read()).hexdigest()[:16]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(), library_sha256=digest, results=[row]), f, indent=1)
    trainer.close()
    est.close()


if __name__ == "__main__":
    main()
