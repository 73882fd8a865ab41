"""What the terrain-estimator runner's collection costs (MEASUREMENT TOOL, not product; needs the GPU).  `elspider_air_rough_raycast` as registered (the
tile proportions fixed as `make_env` of tools/train_estimator.py fixes them), 4096 envs, 24 steps per collection, the estimator of the reference's
script (28 x 56, encoder 64, GRU 256, decoder 128-64), one process, interleaved blocks: every block times each variant once, in turn, so drift hits
all of them alike; the figure of a variant is the median over blocks, the spread the range of the blocks.  Every timed window ends in a device
synchronise.

(a) the new entry against the existing one: `lg_runner_collect_estimation` with a raw-row actor and no stats against `collect_estimation(one_call=True)`
    -- the same loop; reported with whether the new entry's median lies inside the existing entry's own block spread;
(b) the added cost per step of the normaliser's apply, of the recurrent driver (a wide GRU memory in front of the actor) and of the error figures,
    and the error kernel alone over the call's (T, N, R) rows against the 4 T torch reductions `_collect_estimation_one_call` runs;
(c) one runner iteration (`learn(1)`: collection + update) against the loop of `tools/train_estimator.py --collect one-call --update native`;
(d) `play` throughput in env steps per second: the collection with the estimator stepped and the figures on, fp32 and bf16 encoder.

(e) `--training-modes`, a run of its own: one runner iteration (`learn(1)`) with `algorithm.encoder_training` "fp32" and "bf16", two runners on two
    envs in one process, interleaved blocks; merged into the same file under "e_runner_iteration_by_encoder_training".

Writes profiles/native_runner_estimator.json.  usage: python tools/bench_runner_estimator.py [--envs 4096] [--steps 24] [--blocks 7] [--reps 3]"""
import argparse
import datetime
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from extended_legged_gym_amd.native import LIB_PATH  # noqa: E402
from extended_legged_gym_amd.rl import (NativeActorCritic, NativeActorCriticRecurrent, NativeEmpiricalNormalization, NativeEstimatorDistillation,  # noqa: E402
                                        NativeTerrainEstimator, NativeTerrainEstimatorRunner, collect_estimation, collect_estimation_driven, estimation_errors)
from extended_legged_gym_amd.rl.runner import initial_state_dict  # noqa: E402
from extended_legged_gym_amd.scripts.terrain_est_train import create_terrain_estimator_config, get_terrain_estimator_args  # noqa: E402
from train_estimator import make_env  # noqa: E402

TASK = "elspider_air_rough_raycast"


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def summary(samples):
    return dict(median_ms=statistics.median(samples), min_ms=min(samples), max_ms=max(samples), blocks=len(samples))


def torch_reductions(pred, tgt):
    """The 4 T reductions of `_collect_estimation_one_call`."""
    T = pred.shape[0]
    mse, mae = torch.empty(T, device=pred.device), torch.empty(T, device=pred.device)
    for t in range(T):
        mse[t] = torch.mean((pred[t] - tgt[t]) ** 2)
        mae[t] = torch.mean(torch.abs(pred[t] - tgt[t]))
    return mse, mae


def training_modes(a):
    """(e): `learn(1)` of an fp32-trained and of a bf16-trained runner, interleaved."""
    N, T = a.envs, a.steps
    runners = {}
    for mode in ("fp32", "bf16"):
        cfg = create_terrain_estimator_config(get_terrain_estimator_args(["--num_steps_per_env", str(T)]))
        cfg["runner"].update(sensor_collection="native", encoder_precision=mode)
        cfg["algorithm"]["encoder_training"] = mode
        runners[mode] = NativeTerrainEstimatorRunner(make_env(N, small_terrain=a.small_terrain), cfg, log_dir=None, device="cuda:0")
        assert runners[mode].one_call
    for r in runners.values():
        timed(lambda: r.learn(1), 2)
    samples = {mode: [] for mode in runners}
    for _ in range(a.blocks):
        for mode, r in runners.items():
            samples[mode].append(timed(lambda: r.learn(1), a.reps))
    res = {mode: summary(v) for mode, v in samples.items()}
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc["e_runner_iteration_by_encoder_training"] = dict(res, envs=N, steps=T, blocks=a.blocks, reps_per_block=a.reps, small_terrain=bool(a.small_terrain),
                                                          date=datetime.date.today().isoformat(), bf16_over_fp32_median=res["bf16"]["median_ms"] / res["fp32"]["median_ms"],
                                                          last_losses={mode: r.losses[-1] for mode, r in runners.items()})
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["e_runner_iteration_by_encoder_training"], indent=1))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--training-modes", action="store_true", help="(e) only: one runner iteration with encoder_training fp32 and bf16, merged into --out")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small-terrain", action="store_true", help="2 x 3 terrain tiles (a rehearsal, not a figure)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_runner_estimator.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_runner_estimator needs the GPU: a CPU run has no timing to give")
    if a.training_modes:
        return training_modes(a)
    N, T = a.envs, a.steps
    cfg = create_terrain_estimator_config(get_terrain_estimator_args(["--num_steps_per_env", str(T)]))
    cfg["runner"]["sensor_collection"] = "native"
    # (c), and the estimator's weights for everything else: the runner on an env of its own
    runner = NativeTerrainEstimatorRunner(make_env(N, small_terrain=a.small_terrain), cfg, log_dir=None, device="cuda:0")
    assert runner.one_call
    start, shape, R = runner.initial_state_dict, runner.depth_image_shape, runner.num_raycast_outputs
    tool_env = make_env(N, small_terrain=a.small_terrain)
    tool_env.reset()
    trained = NativeTerrainEstimator(start, shape, 6, device="cuda:0")
    alg = NativeEstimatorDistillation(trained, start, **{k: cfg["algorithm"][k] for k in ("num_learning_epochs", "gradient_length", "learning_rate", "max_grad_norm", "loss_type")})

    def tool_iteration():
        drawn = torch.stack([torch.randn(N, tool_env.num_actions, device="cuda") * 0.5 for _ in range(T)])
        with torch.inference_mode():
            rows = collect_estimation(tool_env, None, T, one_call=True, actions=drawn)
        alg.update(rows)
    # (a), (b), (d): one env; the drivers read its 578-column row
    env = make_env(N, small_terrain=a.small_terrain)
    env.reset()
    O, A = env.num_obs, env.num_actions
    policy_cfg = dict(actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], activation="elu", rnn_type="gru", rnn_hidden_size=256, rnn_num_layers=1)
    actor = NativeActorCritic(initial_state_dict("ActorCritic", O, A, policy_cfg, 1), device="cuda:0")
    recurrent = NativeActorCriticRecurrent(initial_state_dict("ActorCriticRecurrent", O, A, policy_cfg, 1), "elu", "gru", device="cuda:0")
    norm = NativeEmpiricalNormalization([O], device="cuda:0").eval()
    est = {p: NativeTerrainEstimator(start, shape, 6, device="cuda:0", encoder_precision=p) for p in ("fp32", "bf16")}
    g = torch.Generator(device="cuda").manual_seed(1)
    pred, tgt = torch.randn(T, N, R, device="cuda", generator=g) * 5, torch.randn(T, N, R, device="cuda", generator=g).abs() * 5
    variants = {
        "existing_one_call": lambda: collect_estimation(env, actor, T, one_call=True),
        "driven_raw_actor": lambda: collect_estimation_driven(env, T, policy=actor),
        "driven_normalised_actor": lambda: collect_estimation_driven(env, T, policy=actor, normalizer=norm),
        "driven_recurrent": lambda: collect_estimation_driven(env, T, policy=recurrent),
        "driven_estimator": lambda: collect_estimation_driven(env, T, policy=actor, estimator=est["fp32"]),
        "driven_estimator_stats": lambda: collect_estimation_driven(env, T, policy=actor, estimator=est["fp32"], stats=True),
        "play_bf16": lambda: collect_estimation_driven(env, T, policy=actor, estimator=est["bf16"], stats=True),
        "errors_kernel_alone": lambda: estimation_errors(pred, tgt),
        "errors_torch_4T_reductions": lambda: torch_reductions(pred, tgt),
        "runner_iteration": lambda: runner.learn(1),
        "tool_loop_iteration": tool_iteration,
    }
    for fn in variants.values():          # warm-up: code objects, allocations, the rig, the trainers' handles
        timed(fn, 2)
    samples = {k: [] for k in variants}
    for _ in range(a.blocks):
        for k, fn in variants.items():
            samples[k].append(timed(fn, a.reps))
    with open(LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:12]
    res = {k: summary(v) for k, v in samples.items()}
    med = {k: v["median_ms"] for k, v in res.items()}
    old, new = res["existing_one_call"], res["driven_raw_actor"]
    out = dict(task=TASK, envs=N, steps=T, blocks=a.blocks, reps_per_block=a.reps, device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(),
               library_sha256_12=lib_hash, small_terrain=bool(a.small_terrain), variants=res,
               a_new_entry_median_inside_existing_spread=bool(old["min_ms"] <= new["median_ms"] <= old["max_ms"]),
               a_new_entry_median_above_existing_max=bool(new["median_ms"] > old["max_ms"]),
               b_added_ms_per_step=dict(normaliser=(med["driven_normalised_actor"] - med["driven_raw_actor"]) / T,
                                        recurrent_driver=(med["driven_recurrent"] - med["driven_raw_actor"]) / T,
                                        stats=(med["driven_estimator_stats"] - med["driven_estimator"]) / T,
                                        errors_kernel_alone=med["errors_kernel_alone"] / T, errors_torch_4T_reductions=med["errors_torch_4T_reductions"] / T),
               c_runner_over_tool_loop_median=med["runner_iteration"] / med["tool_loop_iteration"],
               d_play_env_steps_per_s=dict(fp32=N * T / (med["driven_estimator_stats"] * 1e-3), bf16=N * T / (med["play_bf16"] * 1e-3)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    return out


if __name__ == "__main__":
    main()
