"""What the host costs in a collection that drives the ray caster and the depth camera (MEASUREMENT TOOL, not product; needs the GPU).
`elspider_air_rough_raycast` as registered (the tile proportions fixed as `make_env` of tools/train_estimator.py fixes them), 4096 envs, 24 steps per
collection, one process, interleaved blocks: every block times each variant once, in turn, so drift hits all of them alike; the figure of a
variant is the median over blocks, the spread the range of the blocks.  Every timed window ends in a device synchronise.  The host-loop figures
are the comparison and are measured here, in the same process as the one-call figures.

(a) the runner's collection (`NativeOnPolicyRunner._collect`): the host loop over `env.step` against `lg_runner_collect_sensors`;
(b) `collect_estimation`: the host loop against `lg_collect_estimation`, each without and with an estimator;
(c) one runner iteration (`learn(1)`: collection + update), `sensor_collection` "host" against "native".

Writes profiles/sensor_collection.json.  usage: python tools/bench_sensor_collection.py [--envs 4096] [--steps 24] [--blocks 7] [--reps 3]"""
import argparse
import copy
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
from extended_legged_gym_amd.envs import task_registry  # noqa: E402
from extended_legged_gym_amd.native import LIB_PATH  # noqa: E402
from extended_legged_gym_amd.rl import EpisodeTracker, NativeOnPolicyRunner, NativeTerrainEstimator, collect_estimation  # noqa: E402
from extended_legged_gym_amd.utils.helpers import class_to_dict  # noqa: E402
from train_estimator import TerrainEstimatorTorch, make_env  # noqa: E402

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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small-terrain", action="store_true", help="2 x 3 terrain tiles (a rehearsal, not a figure)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensor_collection.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_sensor_collection needs the GPU: a CPU run has no timing to give")
    N, T = a.envs, a.steps
    train_cfg = copy.deepcopy(class_to_dict(task_registry.get_cfgs(TASK)[1]))
    train_cfg["runner"]["num_steps_per_env"] = T
    variants = {}
    # (a), (c): one env and one runner per way
    runners = {}
    for how in ("host", "native"):
        cfg = copy.deepcopy(train_cfg)
        cfg["runner"]["sensor_collection"] = how
        runners[how] = NativeOnPolicyRunner(make_env(N, small_terrain=a.small_terrain), cfg, log_dir=None, device="cuda:0")
        assert runners[how].layered == (how == "host")
        tracker = EpisodeTracker(N, "cuda:0")
        variants[f"runner_collect_{how}"] = lambda r=runners[how], tr=tracker: r._collect(tr)          # noqa: E731
        variants[f"runner_iteration_{how}"] = lambda r=runners[how]: r.learn(1)          # noqa: E731
    # (b): one env per way; the actor is the runner's own network on the 578-column row
    shape = tuple(runners["host"].env.get_depth_images().shape[-2:])
    R = runners["host"].env.ray_caster.num_rays
    torch.manual_seed(1)
    state = {k: v.detach() for k, v in TerrainEstimatorTorch(shape, 6, R).state_dict().items()}
    keep = []
    for how in ("host", "one_call"):
        env = make_env(N, small_terrain=a.small_terrain)
        env.reset()
        policy = runners["host"].alg.policy
        est = NativeTerrainEstimator(state, shape, 6, device="cuda:0")
        keep.append((env, est))
        variants[f"estimation_{how}"] = lambda env=env, how=how: collect_estimation(env, policy, T, one_call=how == "one_call")          # noqa: E731
        variants[f"estimation_{how}_with_estimator"] = lambda env=env, how=how, est=est: collect_estimation(env, policy, T, estimator=est, one_call=how == "one_call")          # noqa: E731
    for fn in variants.values():          # warm-up: code objects, allocations, the carried rows, the rig
        timed(fn, 2)
    samples = {k: [] for k in variants}
    for _ in range(a.blocks):
        for k, fn in variants.items():
            samples[k].append(timed(fn, a.reps))
    with open(LIB_PATH, "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:12]
    res = {k: summary(v) for k, v in samples.items()}
    pairs = dict(runner_collect=("runner_collect_host", "runner_collect_native"), runner_iteration=("runner_iteration_host", "runner_iteration_native"),
                 estimation=("estimation_host", "estimation_one_call"), estimation_with_estimator=("estimation_host_with_estimator", "estimation_one_call_with_estimator"))
    out = dict(task=TASK, envs=N, steps=T, blocks=a.blocks, reps_per_block=a.reps, device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(),
               library_sha256_12=lib_hash, small_terrain=bool(a.small_terrain), variants=res,
               one_call_below_the_host_loops_minimum={k: res[b]["max_ms"] < res[h]["min_ms"] for k, (h, b) in pairs.items()},
               host_over_one_call_median={k: res[h]["median_ms"] / res[b]["median_ms"] for k, (h, b) in pairs.items()})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    for env, est in keep:
        est.close()
    return out


if __name__ == "__main__":
    main()
