"""Golden vectors for the native PPO update: the reference's vendored rsl_rl (`PPO`, `RolloutStorage`, `ActorCritic`) run in the build container on
torch-CPU, in the style of make_policy_golden.py (fp16-representable parameters, seeded rows).  For two small networks: the filled storage rows,
the permutation `mini_batch_generator` draws (the first draw of `update()`: re-seed, call `torch.randperm` as it does), and after `update()` the loss
dict, the learning rate of every optimiser step, the final learning rate and the state dict.

  mb1   ELU, scalar std, fixed schedule, 1 mini-batch x 2 epochs (the result does not depend on the permutation), entropy bonus
  mb3   tanh, log std, separate critic observations, adaptive schedule, 3 mini-batches x 2 epochs

The rows come from tests/ppo_reference.craft_rows; the seed of mb3 is the first one at which the float64 restatement keeps every mini-batch's KL 5 %
away from both thresholds and moves the learning rate both up and down (what tests/test_ppo_update_reference.py asserts).  Data only."""
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
from rsl_rl.algorithms import PPO  # noqa: E402
from rsl_rl.modules import ActorCritic  # noqa: E402
from rsl_rl.storage import RolloutStorage  # noqa: E402
from tests import ppo_reference as ref  # noqa: E402

CASES = {
    "mb1": dict(net=dict(num_actor_obs=11, num_critic_obs=11, num_actions=6, actor_hidden_dims=[24], critic_hidden_dims=[18, 10], activation="elu",
                         init_noise_std=0.8, noise_std_type="scalar"),
                T=4, N=32, ppo=dict(num_learning_epochs=2, num_mini_batches=1, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3,
                                    schedule="fixed", desired_kl=0.01, max_grad_norm=1.0, use_clipped_value_loss=True), craft=dict(kl_scale=0.05)),
    "mb3": dict(net=dict(num_actor_obs=13, num_critic_obs=17, num_actions=5, actor_hidden_dims=[20, 9], critic_hidden_dims=[12], activation="tanh",
                         init_noise_std=0.6, noise_std_type="log"),
                T=6, N=35, ppo=dict(num_learning_epochs=2, num_mini_batches=3, clip_param=0.2, value_loss_coef=0.7, entropy_coef=0.0, learning_rate=6e-3,
                                    schedule="adaptive", desired_kl=0.004, max_grad_norm=0.5, use_clipped_value_loss=True), craft=dict(kl_scale=0.02)),
}


def hyper_of(ppo):
    return {k: ppo[k] for k in ref.HYPER}


def main():
    out = {}
    for name, case in CASES.items():
        for seed in range(200):
            torch.manual_seed(seed)
            ac = ActorCritic(**case["net"])
            with torch.no_grad():
                for p_ in ac.parameters():
                    p_.copy_(p_.to(torch.float16).to(torch.float32))
            params = {k: v.detach().clone() for k, v in ac.state_dict().items()}
            R = case["T"] * case["N"]
            rows = ref.craft_rows(params, case["net"]["activation"], R, seed + 100, **case["craft"])
            hyper, kw = hyper_of(case["ppo"]), case["ppo"]
            torch.manual_seed(seed + 1000)
            perm = torch.randperm(kw["num_mini_batches"] * (R // kw["num_mini_batches"]))
            _, _, _, trace, _ = ref.update(params, case["net"]["activation"], rows, perm, hyper, kw["num_learning_epochs"], kw["num_mini_batches"],
                                           kw["learning_rate"])
            lrs = [kw["learning_rate"]] + [t["learning_rate"] for t in trace]
            up, down = any(b > a for a, b in zip(lrs, lrs[1:])), any(b < a for a, b in zip(lrs, lrs[1:]))
            near = any(abs(t["kl"] - thr) < 0.05 * thr for t in trace for thr in (2.0 * hyper["desired_kl"], hyper["desired_kl"] / 2.0))
            if hyper["schedule"] == "fixed" or (up and down and not near):
                break
        else:
            raise SystemExit(f"{name}: no seed meets the conditions")
        print(name, "seed", seed, "kl", [round(t["kl"], 5) for t in trace], "lr", lrs)
        st = RolloutStorage("rl", case["N"], case["T"], [case["net"]["num_actor_obs"]], [case["net"]["num_critic_obs"]], [case["net"]["num_actions"]], None, "cpu")
        T, N = case["T"], case["N"]
        st.observations[:] = rows["observations"].view(T, N, -1)
        st.privileged_observations[:] = rows["critic_observations"].view(T, N, -1)
        for k in ("actions", "values", "returns", "advantages", "actions_log_prob", "mu", "sigma"):
            getattr(st, k)[:] = rows[k].view(T, N, -1)
        ppo = PPO(ac, device="cpu", **case["ppo"])
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
        out[f"{name}.loss"] = np.array([loss["value_function"], loss["surrogate"], loss["entropy"]], np.float64)
        out[f"{name}.learning_rate"] = np.float64(ppo.learning_rate)
        out[f"{name}.seed"] = np.int64(seed)
        out[f"{name}.config"] = np.array(json.dumps(dict(activation=case["net"]["activation"], noise_std_type=case["net"]["noise_std_type"], ppo=case["ppo"])))
        print(name, loss, ppo.learning_rate)
    path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "ppo_update.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
