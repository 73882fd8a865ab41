"""Golden vectors for the distillation path: the reference's vendored rsl_rl `StudentTeacher`, `StudentTeacherRecurrent` (LSTM and GRU; teacher
recurrent and not) and `Distillation`, run on torch-CPU.  A small module (student obs 20 / teacher obs 24, hidden 40, 2 memory
layers, MLPs [32, 16], 12 actions, 7 rows) is driven for 24 steps through `Distillation.act` / `process_env_step` (`distillation.py:89-105`) with dones
set at two known steps (`process_env_step` ends in `policy.reset(dones)`).  Recorded per case: the inputs, `action_mean`, `privileged_actions` and the
hidden states after each step's act.  Every module is run once more in float64 (`module.double()`): `fp32_vs_fp64_maxabs[t]` is the reference's own
fp32 error at step t over outputs and hidden states, the yardstick of the GPU test's tolerance.  For the feed-forward case one `Distillation.update`
(`distillation.py:107-153`; gradient_length 15, Adam 1e-3, grad clip 1.0) runs on the stored rows: its mean behaviour loss, the per-batch losses, and
the same in float64.  Weights are stored as float16-exact values."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

ref_loader.load_reference()
sys.path.insert(0, os.path.join(ref_loader.REF_ROOT, "rsl_rl"))
from rsl_rl.algorithms import Distillation  # noqa: E402
from rsl_rl.modules import StudentTeacher, StudentTeacherRecurrent  # noqa: E402

T, N, OBS_S, OBS_T, A = 24, 7, 20, 24, 12
RESET_STEPS = (9, 17)          # dones are set at these steps


def hidden_list(hs):
    if hs is None:
        return []
    return [h.detach().numpy().copy() for h in (hs if isinstance(hs, tuple) else (hs,))]


def build(case):
    torch.manual_seed(0)
    if case == "ff":
        p = StudentTeacher(OBS_S, OBS_T, A, student_hidden_dims=[32, 16], teacher_hidden_dims=[32, 16], activation="elu", init_noise_std=0.1)
    else:
        rnn_type, _, tr = case.partition("_")
        p = StudentTeacherRecurrent(OBS_S, OBS_T, A, student_hidden_dims=[32, 16], teacher_hidden_dims=[32, 16], activation="elu", rnn_type=rnn_type,
                                    rnn_hidden_dim=40, rnn_num_layers=2, init_noise_std=0.1, teacher_recurrent=tr == "tr")
    with torch.no_grad():
        for p_ in p.parameters():
            p_.copy_(p_.to(torch.float16).to(torch.float32))
    return p


def drive(policy, obs, tobs, rewards, dones, with_update):
    """Distillation.act -> process_env_step over the T steps; returns the per-step rows (and the update's losses)."""
    dtype = obs.dtype
    alg = Distillation(policy, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=1.0, loss_type="mse", device="cpu")
    alg.init_storage("distillation", N, T, [OBS_S], [OBS_T], [A])
    for name in ("observations", "privileged_observations", "actions", "privileged_actions", "rewards", "dones"):
        setattr(alg.storage, name, getattr(alg.storage, name).to(dtype))
    rows = dict(mean=[], teacher=[], hid_s=[], hid_t=[])
    torch.manual_seed(5)
    for t in range(T):
        alg.act(obs[t], tobs[t])
        rows["mean"].append(policy.action_mean.detach().numpy().copy())
        rows["teacher"].append(alg.transition.privileged_actions.numpy().copy())
        hs = policy.get_hidden_states()
        rows["hid_s"].append(hidden_list(hs[0] if hs is not None else None))
        rows["hid_t"].append(hidden_list(hs[1] if hs is not None else None))
        alg.process_env_step(rewards[t], dones[t], {})
    if with_update:
        per_batch = []
        inner = alg.loss_fn
        alg.loss_fn = lambda a, b: (lambda l: (per_batch.append(float(l.item())), l)[1])(inner(a, b))
        rows["update_loss"] = alg.update()["behavior"]
        rows["update_per_batch"] = np.array(per_batch)
    return rows


out = {"meta.reset_steps": np.array(RESET_STEPS)}
g = torch.Generator().manual_seed(1)
obs, tobs = torch.randn(T, N, OBS_S, generator=g), torch.randn(T, N, OBS_T, generator=g)
rewards = torch.randn(T, N, generator=g)
dones = torch.zeros(T, N)
dones[RESET_STEPS[0], [1, 4]] = 1.0
dones[RESET_STEPS[1], [0, 4, 6]] = 1.0
out["obs"], out["tobs"], out["rewards"], out["dones"] = obs.numpy(), tobs.numpy(), rewards.numpy(), dones.numpy()
for case in ("ff", "lstm", "gru", "lstm_tr", "gru_tr"):
    policy = build(case)
    for k, v in policy.state_dict().items():
        out[f"{case}.sd.{k}"] = v.detach().numpy().astype(np.float16)
    upd = case == "ff"
    r32 = drive(copy.deepcopy(policy), obs, tobs, rewards, dones, upd)
    r64 = drive(copy.deepcopy(policy).double(), obs.double(), tobs.double(), rewards.double(), dones.double(), upd)
    gap = np.zeros(T)
    for t in range(T):
        pairs = [(r32["mean"][t], r64["mean"][t]), (r32["teacher"][t], r64["teacher"][t])]
        pairs += list(zip(r32["hid_s"][t], r64["hid_s"][t])) + list(zip(r32["hid_t"][t], r64["hid_t"][t]))
        gap[t] = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in pairs)
    out[f"{case}.action_mean"], out[f"{case}.privileged_actions"] = np.stack(r32["mean"]), np.stack(r32["teacher"])
    for mem in ("s", "t"):
        for j, tag in enumerate(("h", "c")[:len(r32["hid_" + mem][0])]):
            out[f"{case}.{tag}_{mem}"] = np.stack([r[j] for r in r32["hid_" + mem]])      # (T, L, N, H): the state after step t's act
    out[f"{case}.fp32_vs_fp64_maxabs"] = gap
    print(case, "fp32 vs fp64 max |diff| over the steps: %.3g" % gap.max())
    if upd:
        out[f"{case}.update_loss"] = np.float64(r32["update_loss"])
        out[f"{case}.update_loss_fp64"] = np.float64(r64["update_loss"])
        out[f"{case}.update_per_batch"] = r32["update_per_batch"]
        out[f"{case}.update_per_batch_fp64"] = r64["update_per_batch"]
        print("update: behaviour loss %.9g (float64 %.12g), per-batch max |diff| %.3g" % (r32["update_loss"], r64["update_loss"],
                                                                                        np.abs(r32["update_per_batch"] - r64["update_per_batch"]).max()))
path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "policy_distillation.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path) // 1024, "KiB")
