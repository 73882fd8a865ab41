"""Task registry with the reference's interface (`utils/task_registry.py:44-155`): `register`, `get_cfgs`, `make_env`,
`make_alg_runner`.  The PPO runner is the external `rsl_rl` package (unchanged caller of this env; imported only when a runner is
requested) or, with `--runner native`, `rl.NativeOnPolicyRunner`: the same surface over the native collection and PPO update
(`rl.NativeDistillationRunner` where the train config's algorithm is `Distillation`)."""
import os
from datetime import datetime
from typing import Tuple

from extended_legged_gym_amd import LEGGED_GYM_ROOT_DIR
from .helpers import class_to_dict, get_args, get_load_path, parse_sim_params, set_seed, update_cfg_from_args


class TaskRegistry():
    def __init__(self):
        self.task_classes = {}
        self.env_cfgs = {}
        self.train_cfgs = {}

    def register(self, name: str, task_class, env_cfg, train_cfg):
        self.task_classes[name] = task_class
        self.env_cfgs[name] = env_cfg
        self.train_cfgs[name] = train_cfg

    def get_task_class(self, name: str):
        return self.task_classes[name]

    def get_cfgs(self, name) -> Tuple[object, object]:
        train_cfg, env_cfg = self.train_cfgs[name], self.env_cfgs[name]
        env_cfg.seed = train_cfg.seed
        return env_cfg, train_cfg

    def make_env(self, name, args=None, env_cfg=None):
        if args is None:
            args = get_args()
        if name not in self.task_classes:
            raise ValueError(f"Task with name: {name} was not registered")
        task_class = self.get_task_class(name)
        if env_cfg is None:
            env_cfg, _ = self.get_cfgs(name)
        env_cfg, _ = update_cfg_from_args(env_cfg, None, args)
        set_seed(env_cfg.seed)
        sim_params = parse_sim_params(args, {"sim": class_to_dict(env_cfg.sim)})
        env = task_class(cfg=env_cfg, sim_params=sim_params, physics_engine=args.physics_engine,
                         sim_device=args.sim_device, headless=args.headless)
        return env, env_cfg

    def make_alg_runner(self, env, name=None, args=None, train_cfg=None, log_root="default"):
        if args is None:
            args = get_args()
        native = getattr(args, "runner", "rsl_rl") == "native"
        if native:
            from extended_legged_gym_amd.rl import NativeOnPolicyRunner as OnPolicyRunner
        else:
            try:
                from rsl_rl.runners import OnPolicyRunner   # external package, drops in unchanged
            except ImportError as e:
                raise ImportError(f"{e}: the rsl_rl package is not installed; `--runner native` trains and resumes with rl.NativeOnPolicyRunner, "
                                  "which needs no external package") from e
        if train_cfg is None:
            if name is None:
                raise ValueError("Either 'name' or 'train_cfg' must be not None")
            _, train_cfg = self.get_cfgs(name)
        elif name is not None:
            print(f"'train_cfg' provided -> Ignoring 'name={name}'")
        _, train_cfg = update_cfg_from_args(None, train_cfg, args)
        if native and algorithm_class_name(train_cfg) == "Distillation":
            from extended_legged_gym_amd.rl import NativeDistillationRunner as OnPolicyRunner
        if log_root == "default":
            log_root = os.path.join(LEGGED_GYM_ROOT_DIR, 'logs', train_cfg.runner.experiment_name)
            log_dir = os.path.join(log_root, datetime.now().strftime('%b%d_%H-%M-%S') + '_' + train_cfg.runner.run_name)
        elif log_root is None:
            log_dir = None
        else:
            log_dir = os.path.join(log_root, datetime.now().strftime('%b%d_%H-%M-%S') + '_' + train_cfg.runner.run_name)
        cfg_dict = class_to_dict(train_cfg)
        if native and getattr(args, "sensor_collection", None) is not None:          # `--sensor_collection host|native` (rl.NativeOnPolicyRunner)
            cfg_dict["runner"]["sensor_collection"] = args.sensor_collection
        runner = OnPolicyRunner(env, cfg_dict, log_dir, device=args.rl_device)
        if train_cfg.runner.resume:
            resume_path = get_load_path(log_root, load_run=train_cfg.runner.load_run, checkpoint=train_cfg.runner.checkpoint)
            print(f"Loading model from: {resume_path}")
            runner.load(resume_path)
        return runner, train_cfg


def algorithm_class_name(train_cfg):
    """The algorithm a train config names: `algorithm.class_name` where it has one, else `runner.algorithm_class_name` (PPO when neither is set)."""
    return getattr(train_cfg.algorithm, "class_name", None) or getattr(train_cfg.runner, "algorithm_class_name", "PPO")


task_registry = TaskRegistry()
