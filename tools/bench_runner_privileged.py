"""What privileged critic observations cost in the native runner (MEASUREMENT TOOL, not product; needs the GPU).  anymal_c_rough_student as
registered (144-wide history for the actor, the 235-wide row for the critic, noise on), 4096 envs, 24 steps per collection, one process,
interleaved blocks as tools/bench_runner.py: every block times each variant once, in turn, so drift hits all of them alike; the figure of a
variant is the median over blocks, the spread the range of the blocks.  Every timed window ends in a device synchronise.

(a) `lg_obsnorm_step_pair` against two `lg_obsnorm_step` calls on (4096, 144) and (4096, 235) rows, in place, training mode;
(b) one collection: the one-call two-stream collector (`lg_runner_collect_privileged`) against the runner's host loop on the same env class,
    both with the two normalisers and the episode tracker;
(c) one runner iteration (collection + `NativePPO.update`) under the PPO train config of anymal_c_rough.

Writes profiles/native_runner_privileged.json.  usage: python tools/bench_runner_privileged.py [--envs 4096] [--steps 24] [--blocks 7] [--reps 5]"""
import argparse
import copy
import datetime
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from extended_legged_gym_amd.envs import task_registry  # noqa: E402
from extended_legged_gym_amd.rl import EpisodeTracker, NativeEmpiricalNormalization, NativeOnPolicyRunner  # noqa: E402
from extended_legged_gym_amd.utils.helpers import class_to_dict, get_args  # noqa: E402
from tools.bench_runner import summary, timed  # noqa: E402

TASK, TRAIN_CFG_FROM = "anymal_c_rough_student", "anymal_c_rough"


def make_runner(n, steps, seed=1):
    env_cfg = copy.deepcopy(task_registry.get_cfgs(TASK)[0])
    env_cfg.env.num_envs, env_cfg.seed = n, seed
    env, _ = task_registry.make_env(TASK, args=get_args(["--headless", "--sim_device", "cuda:0"]), env_cfg=env_cfg)
    cfg = copy.deepcopy(class_to_dict(task_registry.get_cfgs(TRAIN_CFG_FROM)[1]))
    cfg["runner"].update(num_steps_per_env=steps, empirical_normalization=True)
    return NativeOnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")


def library_hash():
    with open(os.path.join(ROOT, "extended_legged_gym_amd", "csrc", "liblgstep.so"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_runner_privileged.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_runner_privileged needs the GPU: a CPU run has no timing to give")
    N, T = a.envs, a.steps
    # ---- (a) the paired step against two single steps, on rows of the flagship's widths (a step is ~10 us: many per timed window)
    widths = (144, 235)
    g = torch.Generator().manual_seed(1)
    rows = [torch.randn(N, w, generator=g).cuda() for w in widths]
    singles = [NativeEmpiricalNormalization([w], device="cuda:0") for w in widths]
    pair = [NativeEmpiricalNormalization([w], device="cuda:0") for w in widths]
    scratch = [r.clone() for r in rows]

    def two_single():
        for _ in range(T):
            singles[0].normalize_(scratch[0]); singles[1].normalize_(scratch[1])

    def one_pair():
        for _ in range(T):
            pair[0].step_pair(pair[1], scratch[0], scratch[1], inplace=True)
    steps = dict(two_lg_obsnorm_step=two_single, lg_obsnorm_step_pair=one_pair)
    for fn in steps.values():
        timed(fn, 2)
    step_ms = {k: [] for k in steps}
    for _ in range(a.blocks):
        for k, fn in steps.items():
            for s, r in zip(scratch, rows):
                s.copy_(r)
            step_ms[k].append(timed(fn, a.reps))
    # ---- (b) the collectors: one runner per variant, so that none inherits another's episode phase
    one_call, host = make_runner(N, T), make_runner(N, T)
    host.layered = True
    trackers = [EpisodeTracker(N, "cuda:0") for _ in range(2)]
    collectors = dict(one_call_privileged=lambda: one_call._collect(trackers[0]), host_loop=lambda: host._collect(trackers[1]))
    for r in (one_call, host):
        r.train_mode()
    for fn in collectors.values():
        timed(fn, 2)
    collect = {k: [] for k in collectors}
    for _ in range(a.blocks):
        for k, fn in collectors.items():
            collect[k].append(timed(fn, a.reps))
    # ---- (c) the iteration
    runner = make_runner(N, T)
    timed(lambda: runner.learn(1), 2)
    iteration = [timed(lambda: runner.learn(1), a.reps) for _ in range(a.blocks)]
    out = dict(date=datetime.date.today().isoformat(), library_sha256_16=library_hash(), task=TASK, train_cfg_from=TRAIN_CFG_FROM, envs=N, steps=T,
               blocks=a.blocks, reps_per_block=a.reps, device=torch.cuda.get_device_name(0),
               method="one process, interleaved blocks, median over blocks (range = spread), every window ends in a device synchronise",
               normalizer_steps_per_window=T, normalizer={k: summary(v) for k, v in step_ms.items()},
               normalizer_us_per_step={k: statistics.median(v) * 1e3 / T for k, v in step_ms.items()},
               collection={k: summary(v) for k, v in collect.items()},
               collection_us_per_step={k: statistics.median(v) * 1e3 / T for k, v in collect.items()},
               iteration=dict(runner_learn=summary(iteration)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    return out


if __name__ == "__main__":
    main()
