"""Train the terrain estimator (depth image + base velocities -> the ray caster's distances) on rows collected by the native side: the
counterpart of the reference's `legged_gym/scripts/terrain_est_train.py` (`TerrainEstimatorRunner.learn`,
`rsl_rl/runners/terrain_estimator_runner.py:362-479`), in the manner of `tools/train_distill.py`.

* `TerrainEstimatorTorch` (`extended_legged_gym_amd/rl/estimator_torch.py`, imported here under its old name): an own torch restatement of
  `rsl_rl/modules/terrain_estimator.py:13-218` with the SAME parameter names, so checkpoints interchange with the reference's module and with
  `NativeTerrainEstimator`.  `tests/test_estimator_golden.py` pins it to outputs recorded from the reference's module.
* `estimator_update`: `EstimatorDistillation.update` (`rsl_rl/algorithms/distillation.py:277-332`): one chunk = the `num_envs` rows of a step,
  a gradient step every `gradient_length` chunks, the memory carried across chunks and detached after each gradient step, in eager PyTorch
  (`--update torch`, the default); `--update native` runs the same update on the device through `rl.NativeEstimatorDistillation`
  (include/lgestimator_train.h).
* collection: `collect_estimation` (`extended_legged_gym_amd/rl/collector.py`) on `elspider_air_rough_raycast`, as its host loop (`--collect host`,
  the default) or as one call into the library (`--collect one-call`); `--python-loop` collects the same rows with a plain loop over `env.step`
  (the checker).

    python tools/train_estimator.py --iters 50 --envs 1024 [--policy walk_policy.pt] [--out run.json] [--update native]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


from extended_legged_gym_amd.rl.estimator_torch import TerrainEstimatorTorch, _Memory, _activation  # noqa: E402,F401  (the module lives in the package; the runner seeds its estimator from it)


ENCODER_STAGE_ENDS = (2, 4, 6, 8, 10, 12, 14)          # depth_encoder[:end] = stage k: conv + act x 4, pool + flatten, linear + act x 2


def encoder_stages(module, depth_images):
    """The seven stage outputs of `module.depth_encoder` on (n, h, w) images, each the Sequential cut after the stage's last module: four maps
    (n, C, H, W), the pooled rows (n, 1024), (n, 128), (n, encoder_output_dim).  What `NativeConvEncoder.stage` is compared with."""
    out, x = [], depth_images.unsqueeze(1)
    with torch.no_grad():
        for i, layer in enumerate(module.depth_encoder):
            x = layer(x)
            if i + 1 in ENCODER_STAGE_ENDS:
                out.append(x)
    return out


def closed_form_state(module, salt=0):
    """Weights as a closed-form rule of the flat index, no RNG: tensor number j of `module.state_dict()` (in its own order), entry i:
        u = ((2654435761 i + 40503 j + 12345 + 7919 salt) mod 2^32) / 2^32;   value = (2 u - 1) * a,
    a = sqrt(3 / fan_in) for a weight (fan_in = the product of its trailing dimensions), 0.1 for a bias; exact integer arithmetic, then one
    rounding to float32.  `tools/refgen/make_estimator_golden.py` fills the reference's module with it and the tests refill ours, so the
    golden file carries no weights."""
    out = {}
    for j, (key, t) in enumerate(module.state_dict().items()):
        i = np.arange(t.numel(), dtype=np.uint64)
        u = ((i * np.uint64(2654435761) + np.uint64(40503 * j + 12345 + 7919 * salt)) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 2.0 ** 32
        a = np.sqrt(3.0 / float(np.prod(t.shape[1:]))) if t.dim() > 1 else 0.1
        out[key] = torch.from_numpy(((2.0 * u - 1.0) * a).astype(np.float32).reshape(tuple(t.shape)))
    return out


def closed_form_depth(T, n, height, width):
    """Depth images as a closed-form rule (no RNG, nothing to store): a smooth ramp plus a hashed texture, in the camera's normalised [0, 1]:
        d[t, e, y, x] = 0.5 + 0.3 sin(0.21 y + 0.13 x + 0.7 e + 0.4 t) + 0.2 (2 u - 1),  u = ((2654435761 i + 99991) mod 2^32) / 2^32 of the flat index i,
    evaluated in float64 and rounded once to float32."""
    i = np.arange(T * n * height * width, dtype=np.uint64)
    u = ((i * np.uint64(2654435761) + np.uint64(99991)) & np.uint64(0xFFFFFFFF)).astype(np.float64).reshape(T, n, height, width) / 2.0 ** 32
    t, e, y, x = np.meshgrid(np.arange(T), np.arange(n), np.arange(height), np.arange(width), indexing="ij")
    return torch.from_numpy((0.5 + 0.3 * np.sin(0.21 * y + 0.13 * x + 0.7 * e + 0.4 * t) + 0.2 * (2.0 * u - 1.0)).astype(np.float32))


# the cases of tests/golden/terrain_estimator.npz: (name, image, memory, activation); case number = the salt of closed_form_state
GOLDEN_CASES = (("gru_28x56", (28, 56), "gru", "elu"), ("lstm_28x56", (28, 56), "lstm", "elu"), ("gru_58x87", (58, 87), "gru", "elu"),
                ("relu_28x56", (28, 56), "gru", "relu"), ("tanh_28x56", (28, 56), "gru", "tanh"))


def estimator_update(model, optimizer, rows, last_hidden_states=None, gradient_length=15, max_grad_norm=None, use_dones=False):
    """`EstimatorDistillation.update` (`distillation.py:277-332`), one epoch, MSE loss.  rows: the dict of `collect_estimation`.  The reference's
    storage holds all-zero dones, so its update never resets the memory inside a rollout; `use_dones` resets on the real ones instead.
    Returns (mean loss, hidden state to carry into the next update)."""
    model.reset(hidden_states=last_hidden_states)
    model.detach_hidden_states()
    T = rows["depth_images"].shape[0]
    loss, mean, cnt = 0, 0.0, 0
    for t in range(T):
        pred = model.act_inference(rows["depth_images"][t], rows["proprio_data"][t])
        step_loss = nn.functional.mse_loss(pred, rows["raycast_targets"][t])
        loss = loss + step_loss
        mean += step_loss.item()
        cnt += 1
        if cnt % gradient_length == 0:
            optimizer.zero_grad()
            loss.backward()
            if max_grad_norm:
                nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)
            optimizer.step()
            model.detach_hidden_states()
            loss = 0
        if use_dones:
            model.reset(rows["dones"][t].view(-1))
    hidden = model.get_hidden_states()
    model.detach_hidden_states()
    return mean / cnt, model.get_hidden_states() if hidden is not None else None


def make_env(num_envs, seed=1, task="elspider_air_rough_raycast", small_terrain=False):
    """The task with both sensors.  As shipped its tile proportions sum to 0.8 and the terrain generator indexes past the list for the rest
    (tests/test_elspider.py): the last two kinds take the missing share here."""
    import copy
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.utils.helpers import get_args
    env_cfg, _ = task_registry.get_cfgs(task)
    env_cfg = copy.deepcopy(env_cfg)
    env_cfg.terrain.confined_terrain_proportions = [0.0, 0.2, 0.4, 0.4]
    if small_terrain:
        env_cfg.terrain.num_rows, env_cfg.terrain.num_cols = 2, 3
    env_cfg.seed = seed
    env, env_cfg = task_registry.make_env(task, args=get_args(["--num_envs", str(num_envs), "--seed", str(seed)]), env_cfg=env_cfg)
    return env


def collect_python_loop(env, policy, num_steps):
    """The checker of `collect_estimation`: the same rows from a plain loop over the env's own accessors."""
    rows = dict(depth_images=[], proprio_data=[], raycast_targets=[], dones=[])
    for _ in range(num_steps):
        rows["depth_images"].append(env.get_depth_images()[:, -1].clone())
        rows["proprio_data"].append(torch.cat([env.base_lin_vel, env.base_ang_vel], dim=-1))
        rows["raycast_targets"].append(env._get_raycast_distances(normalize=False).clone())
        actions = policy.act_inference(env.obs_buf) if policy is not None else torch.randn(env.num_envs, env.num_actions, device=env.device) * 0.5
        rows["dones"].append(env.step(actions)[3].to(torch.float32).clone())
    return {k: torch.stack(v) for k, v in rows.items()}


def train(iters, envs, steps=24, seed=1, policy_path=None, python_loop=False, lr=1e-3, gradient_length=15, out=None, log=print, small_terrain=False, update_device=None,
          eval_precision=None, update="torch", collect="host", train_precision="fp32"):
    """update_device: where the torch update runs (default: the env's device).  "cpu" makes the update reproducible bit for bit -- the GPU's
    convolution backward is not -- which is what a comparison of two collections needs.  eval_precision: the encoder mode ("fp32" | "bf16") of the
    native estimator that plays the trained module over the closing evaluation steps; None: the training precision, so that what is played is what
    was trained.  update: "torch" (`estimator_update`
    on a `TerrainEstimatorTorch`) or "native" (`rl.NativeEstimatorDistillation`: the update on the device, the weights trained in place in an fp32
    `NativeTerrainEstimator`; update_device does not apply).  collect: "host" (`collect_estimation`'s loop over `env.step`) or "one-call" (the
    same rows through `lg_collect_estimation`, include/lgsensors.h; without a policy the 0.5 * randn actions are drawn before the call, step by
    step, so both ways consume the generator alike).  train_precision: "bf16" (with update "native") trains a `NativeTerrainEstimator` whose
    depth encoder runs in bf16 with `NativeEstimatorDistillation(encoder_training="bf16")`."""
    from extended_legged_gym_amd.rl import NativeActorCritic, NativeEstimatorDistillation, NativeTerrainEstimator, collect_estimation
    if update not in ("torch", "native"):
        raise ValueError(f"update {update!r}: must be torch or native")
    if collect not in ("host", "one-call"):
        raise ValueError(f"collect {collect!r}: must be host or one-call")
    if train_precision not in ("fp32", "bf16") or (train_precision == "bf16" and update != "native"):
        raise ValueError(f"train_precision {train_precision!r}: must be fp32, or bf16 with update native")
    eval_precision = eval_precision or train_precision

    def collect_rows(estimator=None):
        if collect == "host":
            return collect_estimation(env, policy, steps, estimator=estimator)
        drawn = None if policy is not None else torch.stack([torch.randn(env.num_envs, env.num_actions, device=env.device) * 0.5 for _ in range(steps)])
        return collect_estimation(env, policy, steps, estimator=estimator, one_call=True, actions=drawn)
    torch.manual_seed(seed)
    env = make_env(envs, seed, small_terrain=small_terrain)
    policy = None
    if policy_path:
        ck = torch.load(policy_path, map_location="cpu")
        policy = NativeActorCritic(ck.get("model_state_dict", ck), device=str(env.device))
    depth = env.get_depth_images()
    shape, R = tuple(depth.shape[-2:]), env._get_raycast_distances(normalize=False).shape[1]
    udev = torch.device(update_device or env.device)
    model = TerrainEstimatorTorch(shape, 6, R).to(udev)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    hidden, curve = None, []
    trained = alg = None
    if update == "native":
        start = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        trained = NativeTerrainEstimator(start, shape, 6, device=str(env.device), encoder_precision=train_precision)
        alg = NativeEstimatorDistillation(trained, start, gradient_length=gradient_length, learning_rate=lr, encoder_training=train_precision)
    for it in range(iters):
        with torch.inference_mode():
            rows = collect_python_loop(env, policy, steps) if python_loop else collect_rows()
        if alg is not None:
            loss = alg.update(rows)["estimation"]
        else:
            rows = {k: v.to(udev, copy=True) for k, v in rows.items()}
            loss, hidden = estimator_update(model, opt, rows, hidden, gradient_length)
        curve.append(loss)
        log(f"iter {it:4d}  estimation loss {loss:.6f}")
    if alg is not None:
        state = alg.state_dict()
        alg.close()
        trained.close()
    else:
        state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    native = NativeTerrainEstimator(state, shape, 6, device=str(env.device), encoder_precision=eval_precision)          # the file below is one it loads
    with torch.inference_mode():
        ev = collect_rows(native)
    log(f"native estimator ({eval_precision} encoder) over {steps} fresh steps: mse {ev['mse'].mean().item():.6f}  mae {ev['mae'].mean().item():.6f}")
    if out:
        with open(out, "w") as f:
            json.dump(dict(task="elspider_air_rough_raycast", envs=envs, steps=steps, seed=seed, loss=curve, eval_precision=eval_precision, eval_mse=ev["mse"].mean().item(),
                           eval_mae=ev["mae"].mean().item()), f)
        torch.save(dict(model_state_dict=state, depth_image_shape=shape, proprio_dim=6, num_raycast_outputs=R), os.path.splitext(out)[0] + "_model.pt")
    native.close()
    env.core.close()
    return curve


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=24, help="num_steps_per_env of the runner")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--policy", default=None, help="checkpoint of an ActorCritic that drives the robot (default: 0.5 * randn actions)")
    ap.add_argument("--python-loop", action="store_true", help="collect with a plain loop over env.step (the checker of collect_estimation)")
    ap.add_argument("--out", default=None, help="write the loss curve here (JSON) and the trained module next to it (_model.pt)")
    ap.add_argument("--small-terrain", action="store_true", help="2 x 3 terrain tiles (quick runs)")
    ap.add_argument("--eval-precision", choices=("fp32", "bf16"), default=None, help="encoder mode of the native estimator that plays the trained module at the end (default: --train-precision)")
    ap.add_argument("--update", choices=("torch", "native"), default="torch", help="where the gradient steps run: eager torch, or the library's kernels (rl.NativeEstimatorDistillation)")
    ap.add_argument("--collect", choices=("host", "one-call"), default="host", help="collect_estimation as the host loop over env.step, or as one call into the library (lg_collect_estimation)")
    ap.add_argument("--train-precision", choices=("fp32", "bf16"), default="fp32", help="with --update native: bf16 trains the estimator whose depth encoder runs in bf16 (fp32 masters and Adam)")
    a = ap.parse_args(argv)
    train(a.iters, a.envs, a.steps, a.seed, a.policy, a.python_loop, out=a.out, small_terrain=a.small_terrain, eval_precision=a.eval_precision, update=a.update,
          collect=a.collect, train_precision=a.train_precision)


if __name__ == "__main__":
    main()
