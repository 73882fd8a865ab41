"""CPU side of privileged critic observations in the native runner: the initial weights with a critic of its own input width
(`initial_state_dict(..., num_critic_obs=...)`), and the rule that picks the collector for an env with privileged observations
(`collects_privileged_natively`).  No GPU needed."""
import pytest
import torch

CFG = dict(actor_hidden_dims=[64, 32], critic_hidden_dims=[48], activation="elu", init_noise_std=0.7, rnn_type="lstm", rnn_hidden_size=64, rnn_num_layers=1)


@pytest.mark.parametrize("name", ["ActorCritic", "ActorCriticRecurrent"])
def test_critic_input_width(name):
    from extended_legged_gym_amd.rl.runner import initial_state_dict
    base = initial_state_dict(name, 144, 12, CFG, 3)
    wide = initial_state_dict(name, 144, 12, CFG, 3, num_critic_obs=235)
    assert list(wide) == list(base)
    if name == "ActorCritic":
        assert wide["critic.0.weight"].shape == (48, 235) and wide["actor.0.weight"].shape == (64, 144) and base["critic.0.weight"].shape == (48, 144)
    else:
        assert wide["memory_c.rnn.weight_ih_l0"].shape == (4 * 64, 235) and wide["memory_a.rnn.weight_ih_l0"].shape == (4 * 64, 144)
        assert base["memory_c.rnn.weight_ih_l0"].shape == (4 * 64, 144) and wide["critic.0.weight"].shape == (48, 64)
    # the actor is drawn first: the critic's width does not move its bits
    assert all(torch.equal(wide[k], base[k]) for k in base if k.startswith("actor.") or k == "std")
    for same in (None, 144):
        again = initial_state_dict(name, 144, 12, CFG, 3, num_critic_obs=same)
        assert list(again) == list(base) and all(again[k].dtype == base[k].dtype and torch.equal(again[k], base[k]) for k in base)


def test_the_global_generator_is_left_alone():
    from extended_legged_gym_amd.rl.runner import initial_state_dict
    torch.manual_seed(7)
    want = torch.rand(3)
    torch.manual_seed(7)
    initial_state_dict("ActorCritic", 144, 12, CFG, 3, num_critic_obs=235)
    assert torch.equal(torch.rand(3), want)


def test_collector_rule_for_privileged_observations():
    """Only the class whose work around the native step is the history layer the library runs itself collects with the one-call privileged
    collector; `steps_outside_the_library` is what it was (tests/test_runner_checkpoint_layout.py pins it)."""
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.envs.anymal_c.anymal import AnymalStudent
    from extended_legged_gym_amd.envs.base.legged_robot import LeggedRobot
    from extended_legged_gym_amd.rl.runner import collects_privileged_natively, steps_outside_the_library
    native = {name: collects_privileged_natively(object.__new__(cls)) for name, cls in task_registry.task_classes.items()}
    assert native["anymal_c_rough_student"] and AnymalStudent.privileged_native_collection is True
    for name in ("elspider_air_rough_raycast", "pose_anymal_c_flat", "pose_go2_flat", "pose_elspider_air_flat", "anymal_c_batch_rollout",
                 "elspider_air_batch_rollout_flat", "go2_batch_rollout", "foot_track_elspider_air_flat", "anymal_c_flat", "anymal_c_rough", "cassie"):
        assert not native[name], name
    assert [name for name, cls in task_registry.task_classes.items() if native[name]] == [name for name, cls in task_registry.task_classes.items()
                                                                                          if issubclass(cls, AnymalStudent)]
    for name, cls in task_registry.task_classes.items():
        assert steps_outside_the_library(object.__new__(cls)) == (cls.step is not LeggedRobot.step or hasattr(cls, "_after_native")), name
    assert steps_outside_the_library(object.__new__(AnymalStudent))
