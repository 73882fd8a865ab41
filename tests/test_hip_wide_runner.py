"""GPU: `NativeOnPolicyRunner` on `elspider_air_rough_raycast`, the one registered task whose policy observation carries a sensor: rows of 66
proprioceptive columns + 512 ray distances.  The policy is the one the task's train config gives (578-128-64-32-18, `lg_mlp_create_wide`), collected through the host loop
(the ray caster runs between physics and post-physics, outside the library's step) and trained by `NativePPO`.  Small terrain as in
tests/test_hip_estimator.py, 32 envs, 4 steps per env, two iterations, with and without `empirical_normalization`."""
import copy
import math

import pytest
import torch

from tests.test_env_api import make
from tests.test_hip_estimator import ENV_OVER

pytestmark = pytest.mark.gpu
TASK, N, T, PROPRIO = "elspider_air_rough_raycast", 32, 4, 66


def train_cfg(**runner):
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.utils.helpers import class_to_dict
    cfg = copy.deepcopy(class_to_dict(task_registry.get_cfgs(TASK)[1]))
    cfg["runner"].update(dict(num_steps_per_env=T, save_interval=1), **runner)
    cfg["seed"] = 4
    return cfg


@pytest.mark.parametrize("normalization", [False, True], ids=["plain", "empirical_normalization"])
def test_two_iterations_on_the_raycast_task_train_the_ray_columns_and_round_trip(tmp_path, normalization):
    from extended_legged_gym_amd import abi
    from extended_legged_gym_amd.rl import NativeOnPolicyRunner
    from extended_legged_gym_amd.rl.runner import _ActorCritic, initial_state_dict
    cfg = train_cfg(empirical_normalization=normalization)
    env = make(TASK, N, **ENV_OVER)
    assert env.num_obs == PROPRIO + 512 == 578 > abi.MLP_MAX_WIDTH
    runner = NativeOnPolicyRunner(env, cfg, log_dir=str(tmp_path), device="cuda:0")
    policy = runner.alg.policy
    hidden = list(cfg["policy"]["actor_hidden_dims"])
    assert policy.actor.dims == [578] + hidden + [env.num_actions] and policy.critic.dims == [578] + list(cfg["policy"]["critic_hidden_dims"]) + [1]
    assert env.num_actions == 18 and runner.layered          # the network of the task's own train config; the host loop collects
    sd0 = initial_state_dict("ActorCritic", 578, env.num_actions, cfg["policy"], cfg["seed"])
    assert torch.equal(runner.alg.state_dict()["actor.0.weight"], sd0["actor.0.weight"])
    # one collection and one update by hand: finite losses, then the loop itself
    from extended_legged_gym_amd.rl import EpisodeTracker
    rollout = runner._collect(EpisodeTracker(N, "cuda:0"))
    assert rollout["observations"].shape == (T, N, 578) and bool(torch.isfinite(rollout["observations"]).all())
    assert float(rollout["observations"][..., PROPRIO:].abs().max()) > 0.0          # the rays are in the row
    loss = runner.alg.update(rollout)
    print("losses", loss)
    assert all(math.isfinite(v) for v in loss.values()), loss
    runner.learn(2)
    sd = runner.alg.state_dict()
    moved = (sd["actor.0.weight"] - sd0["actor.0.weight"]).abs()
    print("largest move of a proprioceptive column", float(moved[:, :PROPRIO].max()), "of a ray column", float(moved[:, PROPRIO:].max()))
    assert float(moved[:, PROPRIO:512].max()) > 0.0 and float(moved[:, 512:].max()) > 0.0          # ray columns on both sides of the slab edge train
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    # the checkpoint: rsl_rl's layout, loads into the torch module, and a fresh runner acts with equal bits
    path = str(tmp_path / "model_1.pt")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert [k for k in ck if "norm" not in k] == ["model_state_dict", "optimizer_state_dict", "iter", "infos"]
    assert ("obs_norm_state_dict" in ck) == normalization
    if normalization:
        assert ck["obs_norm_state_dict"]["_mean"].numel() == 578
    module = _ActorCritic(578, env.num_actions, hidden, cfg["policy"]["critic_hidden_dims"], cfg["policy"].get("activation", "elu"),
                          float(cfg["policy"].get("init_noise_std", 1.0)), "scalar")
    module.load_state_dict(ck["model_state_dict"])
    assert list(module.actor[0].weight.shape) == [hidden[0], 578]
    fresh = NativeOnPolicyRunner(make(TASK, N, **ENV_OVER), cfg, device="cuda:0")
    fresh.load(path)
    x = rollout["observations"].reshape(T * N, 578)
    ya, yb = runner.get_inference_policy(device="cuda:0")(x), fresh.get_inference_policy()(x)
    assert torch.equal(ya, yb) and ya.shape == (T * N, 18)
