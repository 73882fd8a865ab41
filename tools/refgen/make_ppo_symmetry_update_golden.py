"""Golden vectors for the native PPO update with `symmetry_cfg`: the reference's vendored rsl_rl (`PPO`, `RolloutStorage`, `ActorCritic`) run in the
build container on torch-CPU with the reference's OWN `get_symmetric_observation_action` of ElSpider Air (66-wide rows, 18 actions), in the format of
make_ppo_update_golden.py plus `symmetry` as the fourth loss and the three plain keys of the `symmetry_cfg` in the config.

  mirror    use_mirror_loss only (the setting elspider_air_rough_train_config.py ships, coefficient 0.6), fixed schedule, 2 mini-batches x 2 epochs
  augment   use_data_augmentation only, fixed schedule, log std, 1 mini-batch x 2 epochs, entropy bonus
  both      both, adaptive schedule, 3 mini-batches x 2 epochs: the first seed at which the float64 restatement keeps the KL of the ORIGINAL rows 5 %
            clear of both thresholds at every step, moves the learning rate both ways, and at which the KL over all K B rows would fall on the other
            side of a threshold at least once (what tests/test_ppo_symmetry_reference.py asserts)
Every case takes the first seed at which the update's mean surrogate loss is at least 0.03 in magnitude (its steps' values are of that size and of
both signs; a mean that nearly cancels cannot be held to a relative tolerance).

The rows come from tests/ppo_reference.craft_rows on the network after tests/ppo_symmetry_reference.calm.  Data only."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

ref_loader.load_reference()
sys.path.insert(0, os.path.join(ref_loader.REF_ROOT, "rsl_rl"))
sys.path.insert(0, ref_loader.REPO_ROOT)
from legged_gym.envs.elspider_air.elspider import get_symmetric_observation_action  # noqa: E402
from rsl_rl.algorithms import PPO  # noqa: E402
from rsl_rl.modules import ActorCritic  # noqa: E402
from rsl_rl.storage import RolloutStorage  # noqa: E402
from tests import ppo_reference as ref  # noqa: E402
from tests import ppo_symmetry_reference as sref  # noqa: E402

NET = dict(num_actor_obs=66, num_critic_obs=66, num_actions=18, actor_hidden_dims=[32, 16], critic_hidden_dims=[24], activation="elu", init_noise_std=0.7)
CASES = {
    "mirror": dict(net=dict(NET, noise_std_type="scalar"), T=4, N=12, symmetry=dict(use_data_augmentation=False, use_mirror_loss=True, mirror_loss_coeff=0.6),
                   ppo=dict(num_learning_epochs=2, num_mini_batches=2, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.0, learning_rate=1e-3,
                            schedule="fixed", desired_kl=0.01, max_grad_norm=1.0, use_clipped_value_loss=True), craft=dict(kl_scale=0.05)),
    "augment": dict(net=dict(NET, noise_std_type="log"), T=4, N=10, symmetry=dict(use_data_augmentation=True, use_mirror_loss=False, mirror_loss_coeff=0.0),
                    ppo=dict(num_learning_epochs=2, num_mini_batches=1, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3,
                             schedule="fixed", desired_kl=0.01, max_grad_norm=1.0, use_clipped_value_loss=True), craft=dict(kl_scale=0.05)),
    "both": dict(net=dict(NET, noise_std_type="scalar"), T=3, N=21, symmetry=dict(use_data_augmentation=True, use_mirror_loss=True, mirror_loss_coeff=0.6),
                 ppo=dict(num_learning_epochs=2, num_mini_batches=3, clip_param=0.2, value_loss_coef=0.7, entropy_coef=0.0, learning_rate=4e-3,
                          schedule="adaptive", desired_kl=0.013, max_grad_norm=0.5, use_clipped_value_loss=True), craft=dict(kl_scale=0.02)),
}


def side(kl, d):
    return 0 if kl > 2.0 * d else (2 if kl < d / 2.0 else 1)


def main():
    out = {}
    for name, case in CASES.items():
        sym = dict(case["symmetry"], data_augmentation_func=get_symmetric_observation_action, _env=None)
        for seed in range(400):
            torch.manual_seed(seed)
            ac = ActorCritic(**case["net"])
            with torch.no_grad():
                for k, v in sref.calm({k: v.detach() for k, v in ac.state_dict().items()}).items():
                    ac.state_dict()[k].copy_(v.to(torch.float16).to(torch.float32))
            params = {k: v.detach().clone() for k, v in ac.state_dict().items()}
            R = case["T"] * case["N"]
            rows = ref.craft_rows(params, case["net"]["activation"], R, seed + 100, share_observations=True, **case["craft"])
            hyper, kw = {k: case["ppo"][k] for k in ref.HYPER}, case["ppo"]
            torch.manual_seed(seed + 1000)
            perm = torch.randperm(kw["num_mini_batches"] * (R // kw["num_mini_batches"]))
            _, loss64, _, trace, _ = sref.update(params, case["net"]["activation"], rows, perm, hyper, sym, kw["num_learning_epochs"], kw["num_mini_batches"],
                                            kw["learning_rate"])
            lrs = [kw["learning_rate"]] + [t["learning_rate"] for t in trace]
            up, down = any(b > a for a, b in zip(lrs, lrs[1:])), any(b < a for a, b in zip(lrs, lrs[1:]))
            d = hyper["desired_kl"]
            near = any(abs(t["kl"] - thr) < 0.05 * thr for t in trace for thr in (2.0 * d, d / 2.0))
            other = any(side(t["kl"], d) != side(t["kl_all"], d) for t in trace)
            # the tests hold the loss means to RELATIVE tolerances: a mean surrogate that is the near-cancellation of its steps' values cannot carry one
            if abs(loss64["surrogate"]) >= 0.03 and (hyper["schedule"] == "fixed" or (up and down and not near and other)):
                break
        else:
            raise SystemExit(f"{name}: no seed meets the conditions")
        print(name, "seed", seed, "kl", [round(t["kl"], 5) for t in trace], "kl_all", [round(t["kl_all"], 5) for t in trace], "lr", lrs)
        st = RolloutStorage("rl", case["N"], case["T"], [case["net"]["num_actor_obs"]], [case["net"]["num_critic_obs"]], [case["net"]["num_actions"]], None, "cpu")
        T, N = case["T"], case["N"]
        st.observations[:] = rows["observations"].view(T, N, -1)
        st.privileged_observations[:] = rows["critic_observations"].view(T, N, -1)
        for k in ("actions", "values", "returns", "advantages", "actions_log_prob", "mu", "sigma"):
            getattr(st, k)[:] = rows[k].view(T, N, -1)
        ppo = PPO(ac, device="cpu", symmetry_cfg=dict(sym), **case["ppo"])
        ppo.storage = st
        trajectory, step = [], ppo.optimizer.step

        def recording_step(*a, **k):          # the learning rate each optimiser step ran with (after the adaptive rule of that mini-batch)
            trajectory.append(ppo.optimizer.param_groups[0]["lr"])
            return step(*a, **k)
        ppo.optimizer.step = recording_step
        torch.manual_seed(seed + 1000)
        loss = ppo.update()
        out[f"{name}.lr_trajectory"] = np.array(trajectory, np.float64)
        for k, v in params.items():
            out[f"{name}.sd0.{k}"] = v.numpy().astype(np.float16)
        for k, v in ac.state_dict().items():
            out[f"{name}.sd1.{k}"] = v.detach().numpy()
        for k in ref.ROW_KEYS:
            out[f"{name}.rows.{k}"] = rows[k].numpy()
        out[f"{name}.perm"] = perm.numpy()
        out[f"{name}.loss"] = np.array([loss["value_function"], loss["surrogate"], loss["entropy"], loss["symmetry"]], np.float64)
        out[f"{name}.learning_rate"] = np.float64(ppo.learning_rate)
        out[f"{name}.seed"] = np.int64(seed)
        out[f"{name}.config"] = np.array(json.dumps(dict(activation=case["net"]["activation"], noise_std_type=case["net"]["noise_std_type"], ppo=case["ppo"],
                                                         symmetry=case["symmetry"])))
        print(name, loss, ppo.learning_rate)
    path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "ppo_symmetry_update.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
