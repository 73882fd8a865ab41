"""Golden data for the native distillation runner: the reference's vendored rsl_rl (`StudentTeacher`, `StudentTeacherRecurrent`) and
`torch.optim.Adam`, run in the build container on torch-CPU.  BUILD-CONTAINER ONLY, like its neighbours.

tests/golden/distillation_runner_layout.json: per policy class (feed-forward, lstm, gru) the ordered (name, shape) list of `named_parameters()`,
the `state_dict()` keys, the optimiser's state after ONE step on a loss through `act_inference` alone (so only the tensors that ever receive a
gradient hold moments: the indices, the dtypes and shapes of an entry, the parameter group), and what `load_state_dict` returns for a PPO-style
key set (`actor.*`, `critic.*`, `std`) and for a student-style one (the module's own).  Names, shapes and settings only."""
import contextlib
import io
import json
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

ref_loader.load_reference()
from rsl_rl.modules import ActorCritic, StudentTeacher, StudentTeacherRecurrent  # noqa: E402

layout = {}
kw = dict(num_student_obs=18, num_teacher_obs=30, num_actions=12, student_hidden_dims=[32, 16], teacher_hidden_dims=[24], activation="elu", init_noise_std=0.5)
cases = ((StudentTeacher, {}), (StudentTeacherRecurrent, dict(rnn_type="lstm", rnn_hidden_dim=20, rnn_num_layers=2)),
         (StudentTeacherRecurrent, dict(rnn_type="gru", rnn_hidden_dim=20, rnn_num_layers=1)))
# the teacher's PPO run: an ActorCritic whose actor has the teacher's shapes (built once, first: StudentTeacher.__init__ overwrites the
# function ActorCritic.__init__ calls)
with contextlib.redirect_stdout(io.StringIO()):
    ppo = ActorCritic(num_actor_obs=kw["num_teacher_obs"], num_critic_obs=kw["num_teacher_obs"], num_actions=kw["num_actions"],
                      actor_hidden_dims=kw["teacher_hidden_dims"], critic_hidden_dims=[8], activation="elu", init_noise_std=1.0)
for cls, extra in cases:
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        policy = cls(**kw, **extra)
    opt = torch.optim.Adam(policy.parameters(), lr=1e-3)
    fresh = opt.state_dict()
    obs = torch.ones(4, kw["num_student_obs"])
    (policy.act_inference(obs) ** 2).sum().backward()
    opt.step()
    osd = opt.state_dict()
    names = [n for n, _ in policy.named_parameters()]
    first = sorted(osd["state"].keys())[0]
    resumed_ppo = policy.load_state_dict(ppo.state_dict())
    resumed_student = policy.load_state_dict(policy.state_dict())
    try:
        policy.load_state_dict({"critic.0.weight": torch.zeros(1)})
        other = "loaded"
    except ValueError as e:
        other = str(e)
    tag = cls.__name__ + ("" if not extra else "_" + extra["rnn_type"])
    layout[tag] = dict(policy_class_name=cls.__name__, policy_cfg=dict(kw, **extra),
                       named_parameters=[[n, list(p.shape)] for n, p in policy.named_parameters()],
                       state_dict_keys=list(policy.state_dict().keys()),
                       fresh_optimizer_state_indices=sorted(fresh["state"].keys()),
                       optimizer_state_keys=sorted(osd.keys()), optimizer_state_indices=sorted(osd["state"].keys()),
                       optimizer_state_names=[names[i] for i in sorted(osd["state"].keys())],
                       optimizer_entry={k: [str(v.dtype), list(v.shape)] for k, v in osd["state"][first].items()}, optimizer_entry_name=names[first],
                       param_group={k: v for k, v in osd["param_groups"][0].items() if k != "params"},
                       param_group_keys=list(osd["param_groups"][0].keys()), params=list(osd["param_groups"][0]["params"]),
                       num_param_groups=len(osd["param_groups"]),
                       ppo_state_dict_keys=list(ppo.state_dict().keys()),
                       load_state_dict_returns=dict(ppo=resumed_ppo, student=resumed_student, other=other))
path = os.path.join(ref_loader.REPO_ROOT, "tests", "golden", "distillation_runner_layout.json")
with open(path, "w") as f:
    json.dump(layout, f, indent=1, sort_keys=True)
print("wrote", path, os.path.getsize(path) // 1024, "KiB")
