"""`python -m extended_legged_gym_amd.scripts.terrain_est_train` (reference `legged_gym/scripts/terrain_est_train.py`): train the terrain estimator
(depth image + base velocities -> the ray caster's distances) with `rl.NativeTerrainEstimatorRunner`.  The reference's argument names and defaults,
its `create_terrain_estimator_config` and `setup_environment_for_terrain_estimation`.  Three differences, on purpose:
`--task` defaults to `elspider_air_rough_raycast` (the reference's default names a task its registry does not hold); the experiment directory
`logs/terrain_estimator_<task>` is created before it is listed (the reference's script fails on a first run there); and three arguments of this
project, `--sensor_collection` (`runner.sensor_collection`: host | native), `--encoder_precision` (`runner.encoder_precision` of `play`) and
`--policy_class_name` (the class of `--pretrained_policy`), which leave the config as the reference builds it when they are not given."""
import argparse
import os
from datetime import datetime

TRAIN_PARAMETERS = [
    {"name": "--task", "type": str, "default": "elspider_air_rough_raycast", "help": "registered task with the depth camera and the ray caster"},
    {"name": "--resume", "action": "store_true", "default": False, "help": "continue from a checkpoint of an earlier run"},
    {"name": "--experiment_name", "type": str, "help": "directory under logs/ (default: terrain_estimator_<task>)"},
    {"name": "--run_name", "type": str, "help": "directory of this run (default: a time stamp)"},
    {"name": "--load_run", "type": str, "help": "run to load from; -1 or absent: the newest"},
    {"name": "--checkpoint", "type": int, "default": -1, "help": "iteration of the estimator_<it>.pt to load; -1: the newest"},
    {"name": "--pretrained_policy", "type": str, "help": "checkpoint of the locomotion policy that moves the robot (default: random actions)"},
    {"name": "--headless", "action": "store_true", "default": False, "help": "no viewer (there is none either way)"},
    {"name": "--rl_device", "type": str, "default": "cuda:0", "help": "device of the env and the estimator, e.g. cuda:0"},
    {"name": "--num_envs", "type": int, "default": 4096, "help": "number of envs"},
    {"name": "--seed", "type": int, "help": "seed of the env, the estimator's initial weights and the random actions"},
    {"name": "--max_iterations", "type": int, "default": 1000, "help": "learning iterations"},
    {"name": "--learning_rate", "type": float, "default": 1e-3, "help": "Adam's learning rate"},
    {"name": "--loss_type", "type": str, "default": "mse", "choices": ["mse", "huber", "l1"], "help": "estimation loss"},
    {"name": "--num_learning_epochs", "type": int, "default": 5, "help": "passes over a collection per update"},
    {"name": "--gradient_length", "type": int, "default": 15, "help": "steps per optimiser step (truncated BPTT length)"},
    {"name": "--num_steps_per_env", "type": int, "default": 24, "help": "steps per env per collection"},
    {"name": "--save_interval", "type": int, "default": 100, "help": "iterations between checkpoints"},
    {"name": "--enable_visualization", "action": "store_true", "default": False, "help": "Accepted and ignored: there is no viewer"},
    {"name": "--visualization_interval", "type": int, "default": 1, "help": "Accepted and ignored: there is no viewer"},
]
NATIVE_PARAMETERS = [
    {"name": "--sensor_collection", "type": str, "choices": ["host", "native"], "default": None,
     "help": "host (the default): collect through env.step; native: the one call into the library (runner.sensor_collection)"},
    {"name": "--encoder_precision", "type": str, "choices": ["fp32", "bf16"], "default": None, "help": "encoder mode of the estimator that play steps (runner.encoder_precision)"},
    {"name": "--encoder_training", "type": str, "choices": ["fp32", "bf16"], "default": None,
     "help": "fp32 (the default), or bf16: train the estimator whose depth encoder runs in bf16, natively (algorithm.encoder_training; needs --encoder_precision bf16)"},
    {"name": "--policy_class_name", "type": str, "default": None, "help": "ActorCritic (the default) or ActorCriticRecurrent: the class of --pretrained_policy"},
]


def build_parser(description, parameters):
    parser = argparse.ArgumentParser(description=description)
    for param in parameters:
        parser.add_argument(param["name"], **{k: v for k, v in param.items() if k != "name"})
    return parser


def device_arguments(args):
    """What `task_registry.make_env` reads beyond the script's own arguments: one device for simulation and learning."""
    args.physics_engine, args.use_gpu_pipeline = "native_hip", True
    args.sim_device = args.rl_device
    args.sim_device_id = int(args.sim_device.split(":")[1]) if ":" in args.sim_device else 0
    args.sim_device_type = args.sim_device.split(":")[0]
    args.num_threads = 0
    return args


def get_terrain_estimator_args(argv=None):
    """Parse command line arguments for terrain estimator training."""
    return device_arguments(build_parser("Terrain Estimator Training", TRAIN_PARAMETERS + NATIVE_PARAMETERS).parse_args(argv))


def create_terrain_estimator_config(args):
    """The reference's function (`terrain_est_train.py:91-125`): the four blocks of the runner's `train_cfg`."""
    train_cfg = {
        "runner": {
            "num_steps_per_env": args.num_steps_per_env,
            "save_interval": args.save_interval,
            "logger": "tensorboard",
            "max_iterations": args.max_iterations,
            "policy_class_name": "ActorCritic",
            "enable_visualization": args.enable_visualization,
            "visualization_interval": args.visualization_interval,
        },
        "algorithm": {
            "num_learning_epochs": args.num_learning_epochs,
            "gradient_length": args.gradient_length,
            "learning_rate": args.learning_rate,
            "max_grad_norm": 1.0,
            "loss_type": args.loss_type,
        },
        "estimator": {
            "encoder_output_dim": 64,
            "memory_hidden_size": 256,
            "memory_num_layers": 1,
            "memory_type": "gru",
            "decoder_hidden_dims": [128, 64],
            "activation": "elu",
        },
        "policy": {
            "init_noise_std": 1.0,
            "actor_hidden_dims": [512, 256, 128],
            "critic_hidden_dims": [512, 256, 128],
            "activation": "elu",
        },
    }
    return native_runner_options(train_cfg, args)


def native_runner_options(train_cfg, args):
    """This project's keys of the `runner` block, each only when its argument is given."""
    for key in ("sensor_collection", "encoder_precision", "policy_class_name"):
        if getattr(args, key, None) is not None:
            train_cfg["runner"][key] = getattr(args, key)
    if getattr(args, "encoder_training", None) is not None:
        train_cfg["algorithm"]["encoder_training"] = args.encoder_training
    if getattr(args, "seed", None) is not None:
        train_cfg["seed"] = args.seed
    return train_cfg


def setup_environment_for_terrain_estimation(env_cfg):
    """Configure environment for terrain estimator training (`terrain_est_train.py:128-146`)."""
    if hasattr(env_cfg, "depth"):
        env_cfg.depth.use_camera = True
        env_cfg.depth.update_interval = 1
        env_cfg.depth.buffer_len = 1
        print("Enabled depth camera for terrain estimation")
    else:
        print("Warning: Environment does not support depth camera")
    if hasattr(env_cfg, "raycaster"):
        env_cfg.raycaster.enable_raycast = True
        print(f"Enabled raycast with {getattr(env_cfg.raycaster, 'num_rays', 'unknown')} rays")
    else:
        print("Warning: Environment does not support raycast")
    # `elspider_air_rough_raycast` ships tile proportions that sum to 0.8, and the terrain generator raises for the tiles beyond them (as the
    # reference's does): the last two kinds take the missing share, the choice of `make_env` in tools/train_estimator.py
    proportions = getattr(getattr(env_cfg, "terrain", None), "confined_terrain_proportions", None)
    if proportions is not None and len(proportions) == 4 and abs(sum(proportions) - 1.0) > 1e-6:
        env_cfg.terrain.confined_terrain_proportions = [0.0, 0.2, 0.4, 0.4]
        print("Terrain tile proportions did not sum to 1: using [0.0, 0.2, 0.4, 0.4]")
    return env_cfg


def experiment_name_of(args):
    return args.experiment_name if args.experiment_name else f"terrain_estimator_{args.task}"


def find_checkpoint(load_path, checkpoint=-1):
    """`estimator_<checkpoint>.pt` of a run directory, the latest for -1; None when the directory holds none."""
    if checkpoint is not None and checkpoint != -1:
        return os.path.join(load_path, f"estimator_{checkpoint}.pt")
    numbers = [int(f.split("_")[1].split(".")[0]) for f in os.listdir(load_path) if f.startswith("estimator_") and f.endswith(".pt")]
    return os.path.join(load_path, f"estimator_{max(numbers)}.pt") if numbers else None


def train_terrain_estimator(args):
    import copy
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.rl import NativeTerrainEstimatorRunner
    print(f"Training terrain estimator for task: {args.task}")
    env_cfg, _ = task_registry.get_cfgs(name=args.task)
    env_cfg = copy.deepcopy(env_cfg)
    if args.num_envs is not None:
        env_cfg.env.num_envs = args.num_envs
    if args.seed is not None:
        env_cfg.seed = args.seed
    env_cfg = setup_environment_for_terrain_estimation(env_cfg)
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    train_cfg = create_terrain_estimator_config(args)
    experiment_dir = os.path.join("logs", experiment_name_of(args))
    os.makedirs(experiment_dir, exist_ok=True)          # (before it is listed: a first run has no such directory)
    earlier = sorted(d for d in os.listdir(experiment_dir) if os.path.isdir(os.path.join(experiment_dir, d)))
    run_name = args.run_name if args.run_name else datetime.now().strftime("%b%d_%H-%M-%S")
    log_dir = os.path.join(experiment_dir, run_name)
    os.makedirs(log_dir, exist_ok=True)
    print(f"Logging to: {log_dir}")
    runner = NativeTerrainEstimatorRunner(env=env, train_cfg=train_cfg, pretrained_policy_path=args.pretrained_policy, log_dir=log_dir, device=args.rl_device)
    if args.resume:
        if args.load_run and args.load_run != "-1":
            load_path = os.path.join(experiment_dir, args.load_run)
        else:
            load_path = os.path.join(experiment_dir, earlier[-1]) if earlier else None
        checkpoint_path = find_checkpoint(load_path, args.checkpoint) if load_path and os.path.isdir(load_path) else None
        if checkpoint_path and os.path.exists(checkpoint_path):
            print(f"Resuming from checkpoint: {checkpoint_path}")
            runner.load(checkpoint_path)
        else:
            print(f"No checkpoint found for resuming in {load_path}")
    print("Starting terrain estimator training...")
    runner.learn(num_learning_iterations=args.max_iterations, init_at_random_ep_len=True)
    print("Training completed!")
    return runner


if __name__ == "__main__":
    try:
        train_terrain_estimator(get_terrain_estimator_args())
    except KeyboardInterrupt as e:
        print(f"Training interrupted: {e}")
