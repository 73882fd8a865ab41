"""Asymmetric actor-critic training with the native runner: PPO on a task whose critic reads privileged observations (needs the GPU).

The reference registers no PPO task with privileged observations; its `anymal_c_rough_student` (history of proprioceptive rows for the
actor, the noise-free row with the height scan as privileged observations) is registered with a Distillation train config.  This tool takes
the env of `--task` and the PPO train config of `--train-cfg-from` (`ActorCritic` + `PPO`; `--policy recurrent`: `ActorCriticRecurrent`), runs
`rl.NativeOnPolicyRunner` on them -- the critic's first layer as wide as `env.num_privileged_obs`, two observation normalisers with
`--empirical-normalization`, the one-call two-stream collector -- and logs to `logs/<experiment>/<run>/`.  No new task is registered.

usage: python tools/train_asymmetric.py [--task anymal_c_rough_student] [--train-cfg-from anymal_c_rough] [--policy feedforward|recurrent]
                                        [--num-envs N] [--iterations K] [--steps-per-env T] [--empirical-normalization] [--seed S]
                                        [--experiment NAME] [--run NAME] [--resume CHECKPOINT]"""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--task", default="anymal_c_rough_student")
    ap.add_argument("--train-cfg-from", default="anymal_c_rough")
    ap.add_argument("--policy", choices=("feedforward", "recurrent"), default="feedforward")
    ap.add_argument("--num-envs", type=int, default=None)
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--steps-per-env", type=int, default=None)
    ap.add_argument("--empirical-normalization", action="store_true")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--experiment", default=None)
    ap.add_argument("--run", default="asymmetric")
    ap.add_argument("--resume", default=None, help="a checkpoint of this runner (or of rsl_rl's OnPolicyRunner on the same env) to continue from")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train_asymmetric needs the GPU: the env and the runner have no CPU path")
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.utils.helpers import get_args
    env_cfg = copy.deepcopy(task_registry.get_cfgs(a.task)[0])
    train_cfg = copy.deepcopy(task_registry.get_cfgs(a.train_cfg_from)[1])
    if a.num_envs is not None:
        env_cfg.env.num_envs = a.num_envs
    if a.seed is not None:
        env_cfg.seed = train_cfg.seed = a.seed
    r = train_cfg.runner
    r.policy_class_name = "ActorCriticRecurrent" if a.policy == "recurrent" else "ActorCritic"
    r.algorithm_class_name = "PPO"
    r.experiment_name = a.experiment or f"asymmetric_{a.task}"
    r.run_name, r.resume = a.run, False
    if a.iterations is not None:
        r.max_iterations = a.iterations
    if a.steps_per_env is not None:
        r.num_steps_per_env = a.steps_per_env
    if a.empirical_normalization:
        r.empirical_normalization = True
    args = get_args(["--headless", "--sim_device", "cuda:0", "--runner", "native"])
    env, _ = task_registry.make_env(a.task, args=args, env_cfg=env_cfg)
    if getattr(env, "num_privileged_obs", None) is None or env.get_privileged_observations() is None:
        raise SystemExit(f"task {a.task} has no privileged observations: scripts/train.py --runner native trains it")
    runner, train_cfg = task_registry.make_alg_runner(env, args=args, train_cfg=train_cfg)
    print(f"actor input {env.num_obs}, critic input {env.num_privileged_obs}; collector: {'host loop' if runner.layered else 'one call'}; log dir {runner.log_dir}")
    if a.resume:
        runner.load(a.resume)
    runner.learn(num_learning_iterations=train_cfg.runner.max_iterations, init_at_random_ep_len=True)
    return runner


if __name__ == "__main__":
    main()
