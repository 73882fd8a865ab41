"""Golden vectors for the recurrent policy kernels: the reference's vendored rsl_rl `ActorCriticRecurrent` (`nn.LSTM` / `nn.GRU` `Memory`
in front of each MLP) run in the build container on torch-CPU.  For `lstm` and `gru` a small module (obs 20 / critic obs 24, hidden 40,
2 layers, MLPs [32, 16], 12 actions, 7 rows) is driven for 24 steps through `act_inference` / `evaluate` with `reset(dones)` at two known
steps and ONE doubled `evaluate` (the state advance of `last_values`, ppo.py:190-192); a twin with the same weights is driven through `act`
for `action_mean`.  Cases `*_x3`: the memory weights scaled by 3 after construction (exactly 3 x the stored float16 values, same inputs:
neither is stored twice), so gates saturate and rounding is fed back harder than with torch's default initialisation.  Every module is evaluated once more in float64 (`module.double()`): `fp32_vs_fp64_maxabs[t]` is the
reference's own fp32 error at step t over outputs and hidden states, the yardstick of the GPU test's tolerance."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

ref_loader.load_reference()
sys.path.insert(0, "/root/reference/rsl_rl")
from rsl_rl.modules import ActorCriticRecurrent  # noqa: E402

T, N, OBS, COBS, A = 24, 7, 20, 24, 12
RESET_STEPS = (9, 17)          # reset(dones) is called after these steps
DOUBLE_EVAL_STEP = 13          # evaluate is called twice on this step's input


def hidden_list(hs):
    return [h.detach().numpy().copy() for h in (hs if isinstance(hs, tuple) else (hs,))]


def drive(ac, obs, cobs, dones, use_act):
    """One pass over the T steps; returns per-step outputs and the hidden states AFTER each step (before that step's reset)."""
    ac.reset()
    rows = dict(inference=[], value=[], value_again=None, mean=[], hid_a=[], hid_c=[])
    with torch.no_grad():
        for t in range(T):
            if use_act:
                ac.act(obs[t])
                rows["mean"].append(ac.action_mean.numpy().copy())
            else:
                rows["inference"].append(ac.act_inference(obs[t]).numpy().copy())
            rows["value"].append(ac.evaluate(cobs[t]).numpy().copy())
            if t == DOUBLE_EVAL_STEP:
                rows["value_again"] = ac.evaluate(cobs[t]).numpy().copy()
            ha, hc = ac.get_hidden_states()
            rows["hid_a"].append(hidden_list(ha)); rows["hid_c"].append(hidden_list(hc))
            if t in RESET_STEPS:
                ac.reset(dones[t])
    return rows


out = {"meta.reset_steps": np.array(RESET_STEPS), "meta.double_eval_step": np.array(DOUBLE_EVAL_STEP)}
for rnn_type in ("lstm", "gru"):
    for scale in (1, 3):
        name = rnn_type if scale == 1 else f"{rnn_type}_x3"
        torch.manual_seed(0)
        ac = ActorCriticRecurrent(OBS, COBS, A, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu", rnn_type=rnn_type,
                                  rnn_hidden_dim=40, rnn_num_layers=2, init_noise_std=0.8)
        with torch.no_grad():
            for k, p_ in ac.named_parameters():
                p_.copy_(p_.to(torch.float16).to(torch.float32))      # stored as float16, still exactly what the reference ran
                if scale != 1 and k.startswith("memory_"):
                    p_.mul_(float(scale))                             # (3 x a float16 value is exact in float32)
        if scale == 1:
            for k, v in ac.state_dict().items():
                out[f"{name}.sd.{k}"] = v.detach().numpy().astype(np.float16)
        g = torch.Generator().manual_seed(1)
        obs, cobs = torch.randn(T, N, OBS, generator=g), torch.randn(T, N, COBS, generator=g)
        dones = torch.zeros(T, N)
        dones[RESET_STEPS[0], [1, 4]] = 1.0
        dones[RESET_STEPS[1], [0, 4, 6]] = 1.0
        r32 = drive(ac, obs, cobs, dones, use_act=False)
        m32 = drive(copy.deepcopy(ac), obs, cobs, dones, use_act=True)
        ac64 = copy.deepcopy(ac).double()
        r64 = drive(ac64, obs.double(), cobs.double(), dones.double(), use_act=False)
        gap = np.zeros(T)
        for t in range(T):
            pairs = [(r32["inference"][t], r64["inference"][t]), (r32["value"][t], r64["value"][t])]
            pairs += list(zip(r32["hid_a"][t], r64["hid_a"][t])) + list(zip(r32["hid_c"][t], r64["hid_c"][t]))
            gap[t] = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in pairs)
        if scale == 1:
            out[f"{name}.obs"], out[f"{name}.cobs"], out[f"{name}.dones"] = obs.numpy(), cobs.numpy(), dones.numpy()
        out[f"{name}.inference"], out[f"{name}.value"] = np.stack(r32["inference"]), np.stack(r32["value"])
        out[f"{name}.value_again"] = r32["value_again"]
        out[f"{name}.mean"] = np.stack(m32["mean"])
        for j, tag in enumerate(("h", "c")[:len(r32["hid_a"][0])]):
            out[f"{name}.{tag}_a"] = np.stack([r[j] for r in r32["hid_a"]])      # (T, L, N, H)
            out[f"{name}.{tag}_c"] = np.stack([r[j] for r in r32["hid_c"]])
        out[f"{name}.fp32_vs_fp64_maxabs"] = gap
        print(name, "fp32 vs fp64 max |diff| over the steps: %.3g" % gap.max())
path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "policy_recurrent.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path) // 1024, "KiB")
