"""GPU: `rl.NativeTerrainEstimatorRunner` with `algorithm.encoder_training = "bf16"` on the small-terrain `elspider_air_rough_raycast`: 64 envs,
8 steps per iteration, `gradient_length` 4.

* `learn` for two iterations trains the estimator with the bf16 encoder that collection predicts with;
* save after two iterations, a fresh runner brought to the same point, `load`, one more iteration: the parameters, both Adam moments, the step count
  and the loss of the uninterrupted run, bit for bit;
* `play` steps the trained object itself and leaves the masters alone;
* a checkpoint written in bf16 mode loads into an fp32 runner and the other way round (the files hold fp32 masters in the reference's layout)."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
N, T, G, SEED = 64, 8, 4, 4


def _cfg(training="bf16", **runner):
    from extended_legged_gym_amd.scripts.terrain_est_train import create_terrain_estimator_config, get_terrain_estimator_args
    cfg = create_terrain_estimator_config(get_terrain_estimator_args(["--num_steps_per_env", str(T), "--gradient_length", str(G), "--num_learning_epochs", "1"]))
    cfg["algorithm"]["encoder_training"] = training
    cfg["runner"].update(dict(sensor_collection="native", encoder_precision=training), **runner)
    cfg["seed"] = SEED
    return cfg


def _env():
    from train_estimator import make_env
    return make_env(N, SEED, small_terrain=True)


def _same_state(a, b):
    assert a["step"] == b["step"] and a["learning_rate"] == b["learning_rate"]
    for part in ("parameters", "exp_avg", "exp_avg_sq"):
        for name in a[part]:
            assert torch.equal(a[part][name], b[part][name]), (part, name)


def test_learn_resume_play_and_checkpoints_across_modes(tmp_path):
    from extended_legged_gym_amd.rl import NativeTerrainEstimatorRunner
    env = _env()
    a = NativeTerrainEstimatorRunner(env, _cfg(save_interval=100), log_dir=str(tmp_path), device="cuda:0")
    assert a.encoder_training == "bf16" and a.estimator.precision == "bf16" and a.alg.encoder_training == "bf16" and a.one_call
    start = {k: v.clone() for k, v in a.alg.state_dict().items()}
    a.learn(2)
    assert a.host_collections == 0 and len(a.losses) == 2 and all(math.isfinite(v) for v in a.losses)
    path = str(tmp_path / "estimator_1.pt")
    assert os.path.exists(path)
    saved = a.alg.optimizer_state()
    assert saved["step"] == 2 * (T // G) and any(not torch.equal(saved["parameters"][k], start[k]) for k in start)
    a.disable_logs = True
    a.learn(1)
    want_loss, want_state = a.losses[-1], a.alg.optimizer_state()
    # a fresh runner on a fresh env, brought to where the first one stood: two collections move the env and the action generator
    env2 = _env()
    b = NativeTerrainEstimatorRunner(env2, _cfg(), log_dir=None, device="cuda:0")
    for _ in range(2):
        b._collect_rows(T)
    b.load(path)
    _same_state(b.alg.optimizer_state(), saved)
    b.learn(1)
    print("next loss, uninterrupted:", want_loss, " resumed:", b.losses[-1])
    assert b.losses[-1] == want_loss
    _same_state(b.alg.optimizer_state(), want_state)
    # play steps the trained object and moves no master
    assert b._estimator_for_play() is b.estimator
    table = b.play(num_episodes=1)
    assert table["rmse"].shape == (b.num_raycast_outputs,) and bool(torch.isfinite(table["rmse"]).all())
    _same_state(b.alg.optimizer_state(), want_state)
    # the file holds fp32 masters: it loads into an fp32 runner, and an fp32 runner's file loads into the bf16 one
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert all(v.dtype == torch.float32 for v in ck["model_state_dict"].values())
    env3 = _env()
    c = NativeTerrainEstimatorRunner(env3, _cfg("fp32", save_interval=100), log_dir=str(tmp_path / "fp32"), device="cuda:0")
    assert c.estimator.precision == "fp32"
    c.load(path)
    _same_state(c.alg.optimizer_state(), saved)
    c.learn(1)
    other = str(tmp_path / "fp32" / f"estimator_{c.current_learning_iteration}.pt")
    c.save(other)
    b.load(other)
    _same_state(b.alg.optimizer_state(), c.alg.optimizer_state())
    b.learn(1)
    assert math.isfinite(b.losses[-1])
    for r in (a, b, c):
        r.close()
    for e in (env, env2, env3):
        e.core.close()
