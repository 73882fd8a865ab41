"""`python -m extended_legged_gym_amd.scripts.terrain_est_play` (reference `legged_gym/scripts/terrain_est_play.py`): load a trained terrain
estimator and run `rl.NativeTerrainEstimatorRunner.play` on it.  The reference's argument names and defaults, with `--task` defaulting to
`elspider_air_rough_raycast` and the runs looked up where `terrain_est_train` writes them (`logs/terrain_estimator_<task>/<run>`; the reference's
play script reads two other directories than its train script writes).  There is no viewer; what play leaves behind is the per-ray error table
(rmse, mae, bias, max per ray), written as JSON next to the checkpoint: `estimator_<it>_per_ray.json`."""
import json
import os

import argparse

from extended_legged_gym_amd.scripts import terrain_est_train
from extended_legged_gym_amd.scripts.terrain_est_train import (NATIVE_PARAMETERS, build_parser, device_arguments, experiment_name_of, find_checkpoint,
                                                                 setup_environment_for_terrain_estimation)

PLAY_PARAMETERS = [
    {"name": "--task", "type": str, "default": "elspider_air_rough_raycast", "help": "registered task with the depth camera and the ray caster"},
    {"name": "--resume", "action": "store_true", "default": False, "help": "continue from a checkpoint of an earlier run"},
    {"name": "--experiment_name", "type": str, "help": "directory under logs/ (default: terrain_estimator_<task>)"},
    {"name": "--run_name", "type": str, "help": "directory of this run (default: a time stamp)"},
    {"name": "--load_run", "type": str, "default": "-1", "help": "run to load from; -1 or absent: the newest"},
    {"name": "--checkpoint", "type": int, "default": -1, "help": "iteration of the estimator_<it>.pt to load; -1: the newest"},
    {"name": "--headless", "action": "store_true", "default": False, "help": "no viewer (there is none either way)"},
    {"name": "--horovod", "action": "store_true", "default": False, "help": "accepted and ignored"},
    {"name": "--rl_device", "type": str, "default": "cuda:0", "help": "device of the env and the estimator, e.g. cuda:0"},
    {"name": "--num_envs", "type": int, "default": 16, "help": "number of envs"},
    {"name": "--seed", "type": int, "help": "seed of the env, the estimator's initial weights and the random actions"},
    {"name": "--max_iterations", "type": int, "help": "learning iterations"},
    {"name": "--num_episodes", "type": int, "default": 10, "help": "episode ends to play until"},
    {"name": "--pretrained_policy", "type": str, "default": None, "help": "checkpoint of the locomotion policy that moves the robot (default: random actions)"},
]
# what create_terrain_estimator_config reads and the play script has no argument for: the training script's defaults
TRAIN_DEFAULTS = dict(num_steps_per_env=24, save_interval=100, max_iterations=1000, enable_visualization=False, visualization_interval=1, num_learning_epochs=5,
                      gradient_length=15, learning_rate=1e-3, loss_type="mse")


def get_terrain_estimator_play_args(argv=None):
    """Parse command line arguments for terrain estimator play."""
    return device_arguments(build_parser("Terrain Estimator Play", PLAY_PARAMETERS + NATIVE_PARAMETERS).parse_args(argv))


def create_terrain_estimator_config(args):
    """The training script's function on the play arguments, the training script's defaults standing in for what play has no argument for."""
    filled = argparse.Namespace(**vars(args))
    for key, value in TRAIN_DEFAULTS.items():
        if getattr(filled, key, None) is None:
            setattr(filled, key, value)
    return terrain_est_train.create_terrain_estimator_config(filled)


def table_as_json(table):
    """The dict `play` returns -> plain lists and numbers."""
    return {k: (v.detach().cpu().tolist() if hasattr(v, "detach") else v) for k, v in table.items()}


def play_terrain_estimator(args):
    import copy
    import torch
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.rl import NativeTerrainEstimatorRunner
    experiment_dir = os.path.join("logs", experiment_name_of(args))
    if args.load_run == "-1":
        runs = sorted(d for d in os.listdir(experiment_dir) if os.path.isdir(os.path.join(experiment_dir, d))) if os.path.isdir(experiment_dir) else []
        if not runs:
            print(f"No previous runs found in {experiment_dir}")
            return None
        log_dir = os.path.join(experiment_dir, runs[-1])
    else:
        log_dir = os.path.join(experiment_dir, args.load_run)
    model_path = find_checkpoint(log_dir, args.checkpoint) if os.path.isdir(log_dir) else None
    if not model_path or not os.path.exists(model_path):
        print(f"No estimator checkpoint found in {log_dir}")
        return None
    print(f"Loading terrain estimator from: {model_path}")
    env_cfg, _ = task_registry.get_cfgs(name=args.task)
    env_cfg = copy.deepcopy(env_cfg)
    env_cfg.env.num_envs = min(args.num_envs if args.num_envs is not None else env_cfg.env.num_envs, 64)
    env_cfg.terrain.num_rows, env_cfg.terrain.num_cols = 5, 5
    env_cfg.terrain.curriculum = False
    env_cfg.terrain.max_init_terrain_level = 0
    env_cfg = setup_environment_for_terrain_estimation(env_cfg)
    # the ray count of the checkpoint's last decoder layer (`terrain_est_play.py:140-160`)
    state = torch.load(model_path, map_location="cpu", weights_only=False)
    state = state.get("model_state_dict", state)
    last = [k for k in state if k.startswith("decoder.") and k.endswith(".weight")][-1]
    print(f"Detected raycast outputs from checkpoint: {state[last].shape[0]}")
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    if env.ray_caster.num_rays != state[last].shape[0]:
        raise ValueError(f"the checkpoint predicts {state[last].shape[0]} distances, the task's ray caster has {env.ray_caster.num_rays} rays")
    runner = NativeTerrainEstimatorRunner(env=env, train_cfg=create_terrain_estimator_config(args), pretrained_policy_path=args.pretrained_policy, log_dir=None,
                                          device=args.rl_device)
    runner.load(model_path, load_optimizer=False)
    print(f"Successfully loaded terrain estimator from iteration {runner.current_learning_iteration}")
    table = runner.play(num_episodes=args.num_episodes, deterministic=True, enable_visualization=False)
    out = os.path.splitext(model_path)[0] + "_per_ray.json"
    with open(out, "w") as f:
        json.dump(table_as_json(table), f)
    print(f"Per-ray error table: {out}")
    return out


if __name__ == "__main__":
    play_terrain_estimator(get_terrain_estimator_play_args())
