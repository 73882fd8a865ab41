"""Golden vectors for the native distillation update: the reference's vendored rsl_rl (`Distillation`, `RolloutStorage("distillation", ...)`,
`StudentTeacher`) run in the build container on torch-CPU, in the style of make_ppo_update_golden.py (fp16-representable parameters, seeded rows).
For two small networks: the filled storage rows and, after `update()`, the returned loss and the state dict.

  g_mse     student 13-20-9-5 ELU, mse, T 7, N 35, G 3, E 1, max_grad_norm 1.0, lr 1e-3: two groups and a one-step remainder
  g_huber   student 11-24-6 tanh, huber, T 4, N 33, G 3, E 2, max_grad_norm None, lr 3e-3: the second group wraps the epoch boundary, two remainder
            steps, no clip

The rows come from tests/distill_reference.craft_rows; the seed of g_huber is the first one at which, in the float64 restatement, every group and
every remainder step has at least 10 % of its elements on each side of the Huber kink and none within 1e-4 of it (what
tests/test_distill_update_reference.py asserts).  Data only."""
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
from rsl_rl.algorithms import Distillation  # noqa: E402
from rsl_rl.modules import StudentTeacher  # noqa: E402
from rsl_rl.storage import RolloutStorage  # noqa: E402
from tests import distill_reference as ref  # noqa: E402

CASES = {
    "g_mse": dict(net=dict(num_student_obs=13, num_teacher_obs=17, num_actions=5, student_hidden_dims=[20, 9], teacher_hidden_dims=[12], activation="elu",
                           init_noise_std=0.1),
                  T=7, N=35, alg=dict(num_learning_epochs=1, gradient_length=3, learning_rate=1e-3, max_grad_norm=1.0, loss_type="mse")),
    "g_huber": dict(net=dict(num_student_obs=11, num_teacher_obs=11, num_actions=6, student_hidden_dims=[24], teacher_hidden_dims=[10, 8], activation="tanh",
                             init_noise_std=0.2),
                    T=4, N=33, alg=dict(num_learning_epochs=2, gradient_length=3, learning_rate=3e-3, max_grad_norm=None, loss_type="huber")),
}


def main():
    out = {}
    for name, case in CASES.items():
        T, N, alg, act = case["T"], case["N"], case["alg"], case["net"]["activation"]
        for seed in range(200):
            torch.manual_seed(seed)
            policy = StudentTeacher(**case["net"])
            with torch.no_grad():
                for p_ in policy.parameters():
                    p_.copy_(p_.to(torch.float16).to(torch.float32))
            sd0 = {k: v.detach().clone() for k, v in policy.state_dict().items()}
            rows = ref.craft_rows(sd0, act, T, N, seed + 100, spread=1.0)
            _, _, trace = ref.update(sd0, act, rows["observations"], rows["privileged_actions"], dtype=torch.float64, **alg)
            fr = [ref.huber_fractions(d) for d in trace["group_diffs"] + trace["rest_diffs"]]
            if alg["loss_type"] != "huber" or all(a >= 0.10 and b >= 0.10 and c >= 1e-4 for a, b, c in fr):
                break
        else:
            raise SystemExit(f"{name}: no seed meets the conditions")
        print(name, "seed", seed, "norms", trace["norms"], "fractions", fr)
        g = torch.Generator().manual_seed(seed + 200)
        st = RolloutStorage("distillation", N, T, [case["net"]["num_student_obs"]], [case["net"]["num_teacher_obs"]], [case["net"]["num_actions"]], None, "cpu")
        st.observations[:] = rows["observations"]
        st.privileged_observations[:] = torch.randn(st.privileged_observations.shape, generator=g)
        st.privileged_actions[:] = rows["privileged_actions"]
        st.actions[:] = rows["privileged_actions"] + 0.1 * torch.randn(st.actions.shape, generator=g)
        st.dones[:] = (torch.rand(T, N, 1, generator=g) < 0.05).byte()
        st.step = T
        algo = Distillation(policy, device="cpu", **alg)
        algo.storage = st
        dones = st.dones.clone()
        loss = algo.update()
        for k, v in sd0.items():
            out[f"{name}.sd0.{k}"] = v.numpy().astype(np.float16)
        for k, v in policy.state_dict().items():
            out[f"{name}.sd1.{k}"] = v.detach().numpy()
        out[f"{name}.observations"] = rows["observations"].numpy()
        out[f"{name}.privileged_actions"] = rows["privileged_actions"].numpy()
        out[f"{name}.dones"] = dones.numpy()
        out[f"{name}.loss"] = np.float64(loss["behavior"])
        out[f"{name}.seed"] = np.int64(seed)
        out[f"{name}.config"] = np.array(json.dumps(dict(activation=act, T=T, N=N, alg=alg)))
        print(name, loss)
    path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "distillation_update.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
