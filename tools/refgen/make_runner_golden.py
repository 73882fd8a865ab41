"""Golden data for the native runner: the reference's vendored rsl_rl (`EmpiricalNormalization`, `ActorCritic`, `ActorCriticRecurrent`) and
`torch.optim.Adam`, run in the build container on torch-CPU.  BUILD-CONTAINER ONLY, like its neighbours.

tests/golden/empirical_normalization.npz: per case of tests/normalizer_reference.py (which regenerates the fp32 input batches from integer arithmetic;
their float64 sums are stored) the module's `_mean`, `_var`, `_std`, `count` after every call and its outputs (the kept rows of the large batches).
tests/golden/runner_checkpoint_layout.json: per policy class and noise type the ordered (name, shape) list of `named_parameters()`, and the key
lists of `optimizer.state_dict()` after one step.  Data only: arrays, names, shapes, settings."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

ref_loader.load_reference()
from rsl_rl.modules import ActorCritic, ActorCriticRecurrent, EmpiricalNormalization  # noqa: E402

sys.path.insert(0, ref_loader.REPO_ROOT)
from tests import normalizer_reference as nr  # noqa: E402

out = {}
for case in nr.CASES:
    name, batches = case["name"], nr.case_batches(case)
    m = EmpiricalNormalization(shape=[case["O"]], eps=case["eps"], until=case["until"])
    rows = torch.from_numpy(nr.kept_rows(case))
    for k in range(case["calls"] + case["eval_calls"]):
        m.train(k < case["calls"])
        x = torch.from_numpy(batches[k])
        with torch.no_grad():
            y = m(x)
        out[f"{name}.xsum{k}"] = np.float64(batches[k].astype(np.float64).sum())
        out[f"{name}.y{k}"] = y[rows].numpy().copy()
        for key in ("_mean", "_var", "_std"):
            out[f"{name}.{key}{k}"] = getattr(m, key).numpy().copy()
        out[f"{name}.count{k}"] = np.int64(int(m.count))
    if case["special"] == "inverse":
        with torch.no_grad():
            out[f"{name}.inv_x"] = m.inverse(torch.from_numpy(batches[-1]))[rows].numpy().copy()
out["cases"] = np.asarray(json.dumps(nr.CASES))
path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "empirical_normalization.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path) // 1024, "KiB")

# ---- the checkpoint layout
layout = {}
kw = dict(num_actor_obs=48, num_critic_obs=48, num_actions=12, actor_hidden_dims=[32, 16], critic_hidden_dims=[24], activation="elu", init_noise_std=1.0)
for cls, extra in ((ActorCritic, {}), (ActorCriticRecurrent, dict(rnn_type="lstm", rnn_hidden_size=20, rnn_num_layers=2)),
                   (ActorCriticRecurrent, dict(rnn_type="gru", rnn_hidden_size=20, rnn_num_layers=1))):
    for noise in ("scalar", "log"):
        torch.manual_seed(0)
        ac = cls(**kw, noise_std_type=noise, **extra)
        opt = torch.optim.Adam(ac.parameters(), lr=1e-3)
        sum((p ** 2).sum() for p in ac.parameters()).backward()
        opt.step()
        osd = opt.state_dict()
        group = {k: v for k, v in osd["param_groups"][0].items() if k != "params"}
        tag = cls.__name__ + ("" if not extra else "_" + extra["rnn_type"]) + "_" + noise
        layout[tag] = dict(policy_class_name=cls.__name__, noise_std_type=noise, policy_cfg=dict(kw, **extra),
                           named_parameters=[[n, list(p.shape)] for n, p in ac.named_parameters()],
                           state_dict_keys=list(ac.state_dict().keys()),
                           optimizer_state_keys=sorted(osd.keys()), optimizer_state_indices=sorted(osd["state"].keys()),
                           optimizer_entry={k: [str(v.dtype), list(v.shape)] for k, v in osd["state"][0].items()},
                           param_group=group, param_group_keys=list(osd["param_groups"][0].keys()), params=list(osd["param_groups"][0]["params"]))
m = EmpiricalNormalization(shape=[48], until=int(1.0e8))
layout["EmpiricalNormalization"] = {k: [str(v.dtype), list(v.shape)] for k, v in m.state_dict().items()}
path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "runner_checkpoint_layout.json")
with open(path, "w") as f:
    json.dump(layout, f, indent=1, sort_keys=True)
print("wrote", path, os.path.getsize(path) // 1024, "KiB")
