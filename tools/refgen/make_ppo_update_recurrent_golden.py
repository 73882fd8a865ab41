"""Golden vectors for the native recurrent PPO update: the reference's vendored rsl_rl (`PPO`, `RolloutStorage`, `ActorCriticRecurrent`) run in the
build container on torch-CPU -- its own padded formulation (`recurrent_mini_batch_generator`, `split_and_pad_trajectories`, `nn.LSTM` / `nn.GRU` over
the padded block, `unpad_trajectories`).  Two cases, `lstm` and `gru`: 2 layers, hidden 40, obs 20 / critic obs 24, MLPs [32, 16], 12 actions,
T = 8, N = 12, 2 epochs x 3 mini-batches, adaptive schedule; dones at (t, env) = (0,1) (7,2) (3,3) (4,3) (6,4) (2,5) (5,5) (1,9) and env 6 done at
every step; memories warmed by one step, so the state at t = 0 is not zero.

The rollout comes from tests/ppo_recurrent_reference.craft_rollout; the seed is the first one at which the float64 restatement keeps every
mini-batch's KL 5 % away from both thresholds, the learning rate moves, and the update's mean surrogate loss is at least 0.03 in magnitude: the
surrogate is a mean of terms -advantage x ratio of magnitude ~1 that largely cancel, its fp32 rounding is about 6e-8 x that magnitude whatever the mean
comes to, and the relative bar of tests/test_ppo_update_reference.py (2e-6 of the recorded mean) only means something above 6e-8 / 2e-6 = 0.03.  Stored: the parameters before (fp16-representable, stored as float16:
exact) and after (float32), the rows, dones, hidden rows, the loss dict, the learning rate every optimiser step ran with.  Data only."""
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
from rsl_rl.modules import ActorCriticRecurrent  # noqa: E402
from rsl_rl.storage import RolloutStorage  # noqa: E402
from tests import ppo_recurrent_reference as rec  # noqa: E402
from tests import ppo_reference as ref  # noqa: E402

T, N, O, OC, A = 8, 12, 20, 24, 12
NET = dict(num_actor_obs=O, num_critic_obs=OC, num_actions=A, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu",
           rnn_hidden_dim=40, rnn_num_layers=2, init_noise_std=0.8)
PPO_KW = dict(num_learning_epochs=2, num_mini_batches=3, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.005, learning_rate=2e-3,
              schedule="adaptive", desired_kl=0.004, max_grad_norm=1.0, use_clipped_value_loss=True)


def main():
    out = {}
    hyper = {k: PPO_KW[k] for k in ref.HYPER}
    for name in ("lstm", "gru"):
        for seed in range(200):
            torch.manual_seed(seed)
            ac = ActorCriticRecurrent(rnn_type=name, **NET)
            with torch.no_grad():
                for p_ in ac.parameters():
                    p_.copy_(p_.to(torch.float16).to(torch.float32))
            params = {k: v.detach().clone() for k, v in ac.state_dict().items()}
            ro = rec.craft_rollout(params, NET["activation"], name, T, N, seed + 100, kl_scale=0.02)
            _, loss64, _, trace, _ = rec.update(params, NET["activation"], name, ro, hyper, PPO_KW["num_learning_epochs"], PPO_KW["num_mini_batches"],
                                           PPO_KW["learning_rate"])
            lrs = [PPO_KW["learning_rate"]] + [t["learning_rate"] for t in trace]
            moved = any(b != a for a, b in zip(lrs, lrs[1:]))
            near = any(abs(t["kl"] - thr) < 0.05 * thr for t in trace for thr in (2.0 * hyper["desired_kl"], hyper["desired_kl"] / 2.0))
            if moved and not near and abs(loss64["surrogate"]) >= 0.03:
                break
        else:
            raise SystemExit(f"{name}: no seed meets the conditions")
        print(name, "seed", seed, "kl", [round(t["kl"], 5) for t in trace], "lr", lrs)
        st = RolloutStorage("rl", N, T, [O], [OC], [A], None, "cpu")
        st.observations[:] = ro["observations"]
        st.privileged_observations[:] = ro["critic_observations"]
        for k in ("actions", "values", "returns", "advantages", "actions_log_prob", "mu", "sigma"):
            getattr(st, k)[:] = ro[k]
        st.dones[:] = ro["dones"].unsqueeze(-1).byte()
        st.saved_hidden_states_a = [ro[k].clone() for k in ("h_a", "c_a") if ro[k] is not None]
        st.saved_hidden_states_c = [ro[k].clone() for k in ("h_c", "c_c") if ro[k] is not None]
        st.step = T
        ppo = PPO(ac, device="cpu", **PPO_KW)
        ppo.storage = st
        trajectory, step = [], ppo.optimizer.step

        def recording_step(*a, **k):          # the learning rate each optimiser step ran with (after the adaptive rule of that mini-batch)
            trajectory.append(ppo.optimizer.param_groups[0]["lr"])
            return step(*a, **k)
        ppo.optimizer.step = recording_step
        loss = ppo.update()
        out[f"{name}.lr_trajectory"] = np.array(trajectory, np.float64)
        for k, v in params.items():
            out[f"{name}.sd0.{k}"] = v.numpy().astype(np.float16)
        for k, v in ac.state_dict().items():
            out[f"{name}.sd1.{k}"] = v.detach().numpy().astype(np.float32)
        for k in rec.ROW_KEYS + ("dones",) + rec.STATE_KEYS:
            if ro[k] is not None:
                out[f"{name}.rollout.{k}"] = ro[k].numpy().astype(np.float32)
        out[f"{name}.loss"] = np.array([loss["value_function"], loss["surrogate"], loss["entropy"]], np.float64)
        out[f"{name}.learning_rate"] = np.float64(ppo.learning_rate)
        out[f"{name}.seed"] = np.int64(seed)
        out[f"{name}.config"] = np.array(json.dumps(dict(activation=NET["activation"], rnn_type=name, noise_std_type="scalar", ppo=PPO_KW)))
        print(name, loss, ppo.learning_rate, trajectory)
    path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "ppo_update_recurrent.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
