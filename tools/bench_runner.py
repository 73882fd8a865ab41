"""What the runner's two device hooks and the runner itself cost (MEASUREMENT TOOL, not product; needs the GPU).  anymal_c_flat, 4096 envs, 24 steps
per collection, one process, interleaved blocks: every block times each variant once, in turn, so drift hits all of them alike; the figure of a
variant is the median over blocks, the spread the range of the blocks.  Every timed window ends in a device synchronise.

(a) one collection: `collect_rollout`, and `collect_rollout_tracked` with the tracker only, the normaliser only (training mode), and both;
(b) one iteration (collection + update): `NativeOnPolicyRunner.learn` against the loop `tools/train_acceptance.py --update native` runs
    (`collect_rollout`, the bookkeeping on the host over the returned rows, `NativePPO.update`).

Writes profiles/native_runner.json.  usage: python tools/bench_runner.py [--envs 4096] [--steps 24] [--blocks 7] [--reps 5]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from extended_legged_gym_amd.envs import task_registry  # noqa: E402
from extended_legged_gym_amd.rl import (EpisodeTracker, NativeActorCritic, NativeEmpiricalNormalization, NativeOnPolicyRunner, NativePPO,  # noqa: E402
                                        collect_rollout, collect_rollout_tracked)
from extended_legged_gym_amd.rl.runner import PPO_KEYS, initial_state_dict  # noqa: E402
from extended_legged_gym_amd.utils.helpers import class_to_dict, get_args  # noqa: E402


def make_env(n, seed=1):
    env_cfg, train_cfg = task_registry.get_cfgs("anymal_c_flat")
    env_cfg = copy.deepcopy(env_cfg)
    env_cfg.env.num_envs, env_cfg.seed = n, seed
    env, _ = task_registry.make_env("anymal_c_flat", args=get_args(["--headless", "--sim_device", "cuda:0"]), env_cfg=env_cfg)
    env.reset()
    return env, copy.deepcopy(class_to_dict(train_cfg))


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_runner.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_runner needs the GPU: a CPU run has no timing to give")
    N, T = a.envs, a.steps
    # ---- (a) the collectors: one env and one policy per variant, so that none inherits another's episode phase
    variants = {}
    for name, (norm, track) in dict(collect_rollout=(None, None), tracked_no_hooks=(False, False), tracker_only=(False, True), normalizer_only=(True, False),
                                    both=(True, True)).items():
        env, cfg = make_env(N)
        sd = initial_state_dict("ActorCritic", env.num_obs, env.num_actions, cfg["policy"], 1)
        pol = NativeActorCritic(sd, cfg["policy"]["activation"], device="cuda:0", seed=1)
        if norm is None:
            fn = lambda env=env, pol=pol: collect_rollout(env, pol, T)          # noqa: E731
        else:
            kw = dict(obs_normalizer=NativeEmpiricalNormalization([env.num_obs], device="cuda:0") if norm else None,
                      episode_tracker=EpisodeTracker(N, "cuda:0") if track else None)
            fn = lambda env=env, pol=pol, kw=kw: collect_rollout_tracked(env, pol, T, **kw)          # noqa: E731
        variants[name] = fn
    for fn in variants.values():          # warm-up: code objects, allocations, the carried row
        timed(fn, 2)
    collect = {k: [] for k in variants}
    for _ in range(a.blocks):
        for k, fn in variants.items():
            collect[k].append(timed(fn, a.reps))
    # ---- (b) the iteration
    env_r, cfg = make_env(N)
    cfg["runner"]["num_steps_per_env"] = T
    runner = NativeOnPolicyRunner(env_r, cfg, log_dir=None, device="cuda:0")
    env_l, _ = make_env(N)
    sd = initial_state_dict("ActorCritic", env_l.num_obs, env_l.num_actions, cfg["policy"], 1)
    pol = NativeActorCritic(sd, cfg["policy"]["activation"], device="cuda:0", seed=1)
    alg = NativePPO(pol, sd, **{k: cfg["algorithm"][k] for k in PPO_KEYS})
    ep_ret, ep_len = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    retbuf, lenbuf = [], []

    def acceptance_iteration():
        nonlocal retbuf, lenbuf
        data = collect_rollout(env_l, pol, T, gamma=cfg["algorithm"]["gamma"], lam=cfg["algorithm"]["lam"])
        rew, dones = data["rewards"][..., 0], data["dones"][..., 0] > 0
        for t in range(T):          # tools/train_acceptance.py: the bookkeeping on the host over the returned rows
            ep_ret.add_(rew[t]); ep_len.add_(1)
            d = dones[t]
            if bool(d.any()):
                retbuf += ep_ret[d].tolist(); lenbuf += ep_len[d].tolist()
                ep_ret[d] = 0; ep_len[d] = 0
        retbuf, lenbuf = retbuf[-100:], lenbuf[-100:]
        alg.update(data)
    iteration = dict(runner_learn=lambda: runner.learn(1), train_acceptance_loop=acceptance_iteration)
    for fn in iteration.values():
        timed(fn, 2)
    iters = {k: [] for k in iteration}
    for _ in range(a.blocks):
        for k, fn in iteration.items():
            iters[k].append(timed(fn, a.reps))
    base = statistics.median(collect["collect_rollout"])
    out = dict(task="anymal_c_flat", envs=N, steps=T, blocks=a.blocks, reps_per_block=a.reps, device=torch.cuda.get_device_name(0),
               collection={k: summary(v) for k, v in collect.items()},
               collection_extra_us_per_step={k: (statistics.median(v) - base) * 1e3 / T for k, v in collect.items() if k != "collect_rollout"},
               iteration={k: summary(v) for k, v in iters.items()})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
    return out


if __name__ == "__main__":
    main()
