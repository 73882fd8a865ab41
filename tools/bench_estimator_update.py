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

`--precision both` compares the two native trainers instead of native against torch: `NativeEstimatorDistillation` with `encoder_training="fp32"` and
with `"bf16"` (include/lgestimator_train_bf16.h) on the same recorded rows, interleaved blocks in one process, median [min, max], and
`workspace_bytes()` of both; the result goes under "precision" of the same JSON.  `--precision bf16 --native-only` is the run a kernel trace of the
bf16 trainer wraps, and `--merge-trace DIR --trace-key bf16_phase_share` files its split.

`--against-lib PATH` checks that the fp32 path of this library costs what another build's does (the parent commit's, say): alternating blocks, each a
fresh child process that loads one of the two libraries (`LGSTEP_LIB`) and times `--reps` fp32 updates; recorded under "fp32_against_lib" with each
side's spread over its blocks.

usage: python tools/bench_estimator_update.py [--reps 5] [--precision fp32 | bf16 | both] [--out profiles/estimator_update.json]"""
import argparse
import csv
import datetime
import glob
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PHASES = (("encoder_forward", ("conv_gemm_kernel", "pool_flatten_kernel", "cat_columns_kernel", "enc_bf16_gemm_kernel", "enc_bf16_pool_kernel", "est16_expand_kernel")),
          ("conv_data_gradient", ("est_dgrad_kernel", "est_pool_backward_kernel", "est16_dgrad_kernel", "est16_pool_backward_kernel")),
          ("conv_weight_gradient", ("est_conv_wgrad_kernel", "est16_wgrad_kernel")),
          ("memory", ("rnn_train_forward_kernel", "rnn_backward_kernel", "rnn_retile_kernel")))


def merge_trace(directory, out, key="native_phase_share"):
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
    stem = key[:-len("_phase_share")] if key.endswith("_phase_share") else key
    doc[key] = {k: v / total for k, v in split.items()}
    doc[stem + "_phase_source"] = "rocprofv3 --kernel-trace --stats, a run of its own (--native-only --reps 2, warm-up included)"
    doc[stem + "_top_kernels_share"] = {k: v / total for k, v in sorted(top.items(), key=lambda kv: -kv[1])[:8]}
    doc[stem + "_traced_kernel_ms"] = total / 1e6
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc[key]))


def _summary(ts):
    return dict(ms_per_update_median=statistics.median(ts), ms_per_update_min=min(ts), ms_per_update_max=max(ts), reps=len(ts))


def against_lib(a):
    """Alternating blocks, one child process each: this library, the other one, this one, ..."""
    blocks = {"this": [], "other": []}
    for block in range(2 * a.blocks):
        side = "this" if block % 2 == 0 else "other"
        env = dict(os.environ)
        if side == "other":
            env["LGSTEP_LIB"] = os.path.abspath(a.against_lib)
        else:
            env.pop("LGSTEP_LIB", None)
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--native-only", "--reps", str(a.reps), "--warmup", str(a.warmup), "--envs", str(a.envs)],
                              env=env, capture_output=True, text=True, check=True, timeout=600)
        row = json.loads([line for line in done.stdout.splitlines() if line.startswith("{")][-1])
        blocks[side].append(row["native"])
        print(side, json.dumps(row["native"]), flush=True)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["fp32_against_lib"] = {side: dict(blocks=rows, median_of_block_medians=statistics.median(r["ms_per_update_median"] for r in rows),
                                          min=min(r["ms_per_update_min"] for r in rows), max=max(r["ms_per_update_max"] for r in rows)) for side, rows in blocks.items()}
    doc["fp32_against_lib"]["other_sha256"] = hashlib.sha256(open(a.against_lib, "rb").read()).hexdigest()[:16]
    doc["fp32_against_lib"]["method"] = "alternating blocks, a fresh process per block; the fp32 trainer of both libraries on the same recorded rows"
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


def precision_run(a, torch, rows, sd, shape, P, G, lr):
    """The fp32 and the bf16 trainer on the same rows (or, with --native-only, the one named), interleaved."""
    from extended_legged_gym_amd.rl import NativeEstimatorDistillation, NativeTerrainEstimator
    sides = ("fp32", "bf16") if a.precision == "both" else (a.precision,)
    ests = {s: NativeTerrainEstimator(sd, shape, P, device="cuda:0", encoder_precision=s) for s in sides}
    algs = {s: NativeEstimatorDistillation(ests[s], sd, gradient_length=G, learning_rate=lr, encoder_training=s) for s in sides}
    times, losses = {s: [] for s in sides}, {s: [] for s in sides}
    for rep in range(a.warmup + a.reps):
        for s in sides:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            loss = algs[s].update(rows)["estimation"]
            e1.record()
            torch.cuda.synchronize()
            losses[s].append(loss)
            if rep >= a.warmup:
                times[s].append(e0.elapsed_time(e1))
    out = {s: dict(_summary(times[s]), workspace_bytes=algs[s].workspace_bytes(), losses=losses[s]) for s in sides}
    if a.precision == "both":
        out["bf16_over_fp32"] = out["bf16"]["ms_per_update_median"] / out["fp32"]["ms_per_update_median"]
        out["workspace_saved_bytes"] = out["fp32"]["workspace_bytes"] - out["bf16"]["workspace_bytes"]
    print(json.dumps({s: {k: v for k, v in r.items() if k != "losses"} if isinstance(r, dict) else r for s, r in out.items()}), flush=True)
    for s in sides:
        algs[s].close(); ests[s].close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--native-only", action="store_true", help="no torch side and no file: the run a kernel trace wraps")
    ap.add_argument("--merge-trace", default=None, help="directory of a rocprofv3 --kernel-trace --stats run: add the per-phase split to --out")
    ap.add_argument("--trace-key", default="native_phase_share", help="with --merge-trace: the key the split is filed under (bf16_phase_share for a bf16 trace)")
    ap.add_argument("--precision", choices=("fp32", "bf16", "both"), default="fp32", help="both: the fp32 and the bf16 trainer interleaved (no torch side); bf16: with --native-only, the traced run")
    ap.add_argument("--against-lib", default=None, help="another build of the library: its fp32 update against this one's, alternating child processes")
    ap.add_argument("--blocks", type=int, default=3, help="with --against-lib: blocks per side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimator_update.json"))
    a = ap.parse_args(argv)
    if a.merge_trace:
        return merge_trace(a.merge_trace, a.out, a.trace_key)
    if a.against_lib:
        return against_lib(a)
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
    g = torch.Generator().manual_seed(1)
    rows = dict(depth_images=closed_form_depth(T, N, *shape).cuda(), proprio_data=torch.randn(T, N, P, generator=g).cuda(),
                raycast_targets=(2.0 + torch.rand(T, N, R, generator=g)).cuda(), dones=torch.zeros(T, N).cuda())
    if a.precision != "fp32":
        result = precision_run(a, torch, rows, sd, shape, P, G, lr)
        if a.native_only or a.precision != "both":
            return
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["precision"] = dict(result, device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(), envs=N, steps=T, gradient_length=G,
                                method="the fp32 and the bf16 trainer on the same recorded rows, interleaved in one process; HIP events around each update")
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
        return
    est = NativeTerrainEstimator(sd, shape, P, device="cuda:0")
    trainer = NativeEstimatorDistillation(est, sd, gradient_length=G, learning_rate=lr)
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
