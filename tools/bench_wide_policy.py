"""The wide input row (`lg_mlp_create_wide`, include/lgpolicy.h) on the clock: what it costs the narrow path, and what the wide path gives.

(a) Narrow path against the parent commit.  `lg_policy_act` at 4096 x 48 and 4096 x 235 (512-256-128) and `NativePPO.update` at 235 (4096 x 24 rows,
    5 epochs x 4 mini-batches) launch the kernel instances the parent launches; only the translation units around them changed.  Each BLOCK is a fresh
    child process (`--narrow-block`) that imports the package from one tree (`--root`): this tree, or a built checkout of the parent commit
    (`--parent-root`), alternating, so both sides see the same machine state.  Per figure: the median over the blocks with [min, max], and the parent's
    own block spread (max - min), which this tree's median may exceed the parent's by at most.
(b) Wide path against eager torch, interleaved in this process: act at 4096 x 578 and the update at 578 (4096 x 24 rows, 5 x 4 mini-batches), networks
    578-512-256-128-18 / -1, ELU.  The figure to read is native / torch.  The act also reports its share of the fp32 matrix peak (2 FLOP per weight
    per row over wall time: an end-to-end rate, launch included).
(c) One iteration of `NativeOnPolicyRunner` on elspider_air_rough_raycast at 4096 envs, collection (the host loop: env.step with the ray caster, one
    `lg_policy_act` per step) and update separately, on the task's terrain grid with confined-terrain proportions that sum to 1.  `--runner-envs 0`
    leaves it out.

Wall clock around a device synchronise; every shape warmed up first.  Synthetic rollout rows for (a) and (b): the cost does not depend on their values.

usage: python tools/bench_wide_policy.py [--parent-root DIR] [--blocks 5] [--reps 7] [--runner-envs 4096] [--out profiles/wide_input.json]"""
import argparse
import datetime
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_MATRIX_PEAK_TFLOPS = 157.3          # MI355X, dense fp32 matrix
T, N, A, E, M = 24, 4096, 12, 5, 4
HIDDEN = [512, 256, 128]
ALG = dict(num_learning_epochs=E, num_mini_batches=M, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3, schedule="adaptive",
           desired_kl=0.01, max_grad_norm=1.0, use_clipped_value_loss=True)


def spread(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts), n=len(ts))


def state_dict(O, num_actions, seed=0):
    """A torch ActorCritic's initial state dict (torch's default nn.Linear initialisation), without the package: both trees build the same one."""
    import torch
    torch.manual_seed(seed)
    sd = {}
    for prefix, dims in (("actor", [O] + HIDDEN + [num_actions]), ("critic", [O] + HIDDEN + [1])):
        for j in range(len(dims) - 1):
            lin = torch.nn.Linear(dims[j], dims[j + 1])
            sd[f"{prefix}.{2 * j}.weight"], sd[f"{prefix}.{2 * j}.bias"] = lin.weight.detach().clone(), lin.bias.detach().clone()
    sd["std"] = torch.ones(num_actions)
    return sd


def rollout_rows(O, num_actions, seed=1):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)          # noqa: E731
    mu = 0.1 * r(T, N, num_actions)
    sigma = torch.ones(T, N, num_actions, device="cuda")
    act = mu + sigma * r(T, N, num_actions)
    logp = torch.distributions.Normal(mu, sigma).log_prob(act).sum(-1, keepdim=True) + 0.1 * r(T, N, 1)
    val = r(T, N, 1)
    return dict(observations=r(T, N, O), actions=act, values=val, returns=val + r(T, N, 1), advantages=r(T, N, 1), actions_log_prob=logp, mu=mu, sigma=sigma)


def timed(fn, reps, warmup):
    import torch
    out = []
    for rep in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def act_loop(policy, obs, calls=2000):
    def go():
        for _ in range(calls):
            policy.act_and_evaluate(obs)
    return go, calls


def narrow_block(root, reps):
    """One block in the tree `root`: median ms of the act (per call) at 48 and 235 and of the update at 235."""
    sys.path.insert(0, root)
    import torch
    from extended_legged_gym_amd.rl import NativeActorCritic, NativePPO
    out = {}
    for O in (48, 235):
        sd = state_dict(O, A)
        policy = NativeActorCritic(sd, "elu", device="cuda:0", seed=1)
        obs = torch.randn(N, O, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
        go, calls = act_loop(policy, obs)
        out[f"act_{O}_us"] = statistics.median(timed(go, reps, 2)) / calls * 1e3
        if O == 235:
            trainer, data = NativePPO(policy, sd, **ALG), rollout_rows(O, A)
            out["update_235_ms"] = statistics.median(timed(lambda: trainer.update(data), reps, 2))
            trainer.close()
    print("BLOCK " + json.dumps(out), flush=True)


def run_block(root, reps):
    env = dict(os.environ, LGSTEP_LIB=os.path.join(root, "extended_legged_gym_amd", "csrc", "liblgstep.so"))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--narrow-block", "--root", root, "--reps", str(reps)], env=env, capture_output=True, text=True,
                       timeout=300)
    lines = [l for l in p.stdout.splitlines() if l.startswith("BLOCK ")]
    if p.returncode != 0 or not lines:
        raise RuntimeError(f"block in {root} failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads(lines[-1][6:])


def narrow_against_parent(parent_root, blocks, reps):
    sides = {"this": HERE, "parent": parent_root}
    got = {k: [] for k in sides}
    for b in range(blocks):
        for k in (("this", "parent") if b % 2 == 0 else ("parent", "this")):
            got[k].append(run_block(sides[k], reps))
            print(k, json.dumps(got[k][-1]), flush=True)
    rows = {}
    for key in got["this"][0]:
        mine, theirs = spread([b[key] for b in got["this"]]), spread([b[key] for b in got["parent"]])
        margin = theirs["max"] - theirs["min"]
        rows[key] = dict(this=mine, parent=theirs, parent_block_spread=margin, this_minus_parent=mine["median"] - theirs["median"],
                         within_parent_spread=bool(mine["median"] - theirs["median"] <= margin))
    return rows


def wide_against_torch(reps):
    import torch
    sys.path.insert(0, os.path.join(HERE, "tools"))
    from train_acceptance import ActorCritic, ppo_update
    from extended_legged_gym_amd.rl import NativeActorCritic, NativePPO
    O, num_actions = 578, 18
    torch.manual_seed(0)
    ac = ActorCritic(O, num_actions, HIDDEN, HIDDEN, 1.0).cuda()
    opt = torch.optim.Adam(ac.parameters(), lr=1e-3)
    sd = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    policy = NativeActorCritic(sd, "elu", device="cuda:0", seed=1)
    trainer, data = NativePPO(policy, sd, **ALG), rollout_rows(O, num_actions)
    obs = data["observations"][0].contiguous()

    def torch_act(calls=2000):
        with torch.no_grad():
            for _ in range(calls):
                mu = ac.actor(obs)
                dist = torch.distributions.Normal(mu, ac.std.expand_as(mu))
                a = dist.sample()
                dist.log_prob(a).sum(-1), ac.critic(obs)
    go, calls = act_loop(policy, obs)
    lr = [1e-3]

    def torch_update():
        lr[0], _ = ppo_update(ac, opt, data, ALG, lr[0])
    times = {k: [] for k in ("act_native", "act_torch", "update_native", "update_torch")}
    for rep in range(2 + reps):
        for key, fn in (("act_native", go), ("act_torch", torch_act), ("update_native", lambda: trainer.update(data)), ("update_torch", torch_update)):
            ts = timed(fn, 1, 0)
            if rep >= 2:
                times[key] += ts
    weights = sum(v.numel() for k, v in sd.items() if k.endswith("weight"))
    act = {k: spread([t / calls * 1e3 for t in times["act_" + k]]) for k in ("native", "torch")}          # us per call
    upd = {k: spread(times["update_" + k]) for k in ("native", "torch")}                                 # ms per update
    tflops = 2.0 * weights * N / (act["native"]["median"] * 1e-6) / 1e12
    trainer.close()
    return dict(networks=[O] + HIDDEN + [num_actions], rows=N,
                act=dict(us_per_call=act, native_over_torch=act["native"]["median"] / act["torch"]["median"], tflops=tflops,
                         fraction_of_fp32_matrix_peak=tflops / FP32_MATRIX_PEAK_TFLOPS),
                update=dict(ms_per_update=upd, rows=T * N, epochs=E, mini_batches=M, native_over_torch=upd["native"]["median"] / upd["torch"]["median"]))


def runner_iteration(envs, reps):
    import copy
    import torch
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.rl import EpisodeTracker, NativeOnPolicyRunner
    from extended_legged_gym_amd.utils.helpers import class_to_dict, get_args
    task = "elspider_air_rough_raycast"
    env_cfg, train_cfg = task_registry.get_cfgs(task)
    env_cfg = copy.deepcopy(env_cfg)
    env_cfg.env.num_envs = envs
    # as registered the task's four confined-terrain proportions sum to 0.8 and a tile choice above that raises (in the reference too): the list of
    # tests/test_hip_estimator.py, which sums to 1, on the task's full terrain grid
    env_cfg.terrain.confined_terrain_proportions = [0.0, 0.2, 0.4, 0.4]
    env, _ = task_registry.make_env(task, args=get_args(["--headless", "--num_envs", str(envs)]), env_cfg=env_cfg)
    cfg = copy.deepcopy(class_to_dict(train_cfg))
    runner = NativeOnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    tracker = EpisodeTracker(envs, "cuda:0")
    collect, update = [], []
    for rep in range(1 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rollout = runner._collect(tracker)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        runner.alg.update(rollout)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep >= 1:
            collect.append((t1 - t0) * 1e3)
            update.append((t2 - t1) * 1e3)
    return dict(task=task, envs=envs, steps_per_env=runner.num_steps_per_env, policy=runner.alg.policy.actor.dims, host_loop=bool(runner.layered),
                collection_ms=spread(collect), update_ms=spread(update))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--narrow-block", action="store_true", help="child mode: one block of the narrow figures in the tree --root")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit; without it part (a) is left out")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--runner-envs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "wide_input.json"))
    a = ap.parse_args(argv)
    if a.narrow_block:
        return narrow_block(a.root, a.reps)
    sys.path.insert(0, HERE)
    lib = os.path.join(HERE, "extended_legged_gym_amd", "csrc", "liblgstep.so")
    out = dict(date=datetime.date.today().isoformat(), library_sha256=hashlib.sha256(open(lib, "rb").read()).hexdigest(),
               fp32_matrix_peak_tflops=FP32_MATRIX_PEAK_TFLOPS, method="wall clock around a device synchronise; medians with [min, max]; sides interleaved")
    if a.parent_root:          # the blocks are child processes: they run before this process opens the device
        out["narrow_against_parent"] = narrow_against_parent(os.path.abspath(a.parent_root), a.blocks, a.reps)
        print(json.dumps(out["narrow_against_parent"]), flush=True)
    import torch
    out["device"] = torch.cuda.get_device_name(0)
    out["wide_against_torch"] = wide_against_torch(a.reps)
    print(json.dumps(out["wide_against_torch"]), flush=True)
    if a.runner_envs > 0:
        out["runner_iteration"] = runner_iteration(a.runner_envs, 3)
        print(json.dumps(out["runner_iteration"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
