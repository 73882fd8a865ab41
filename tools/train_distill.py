"""Teacher-student distillation over the native env and the native collection (`lg_collect_distillation`: act -> lg_step -> history layer, 24 steps
per call), with the hyper-parameters of `AnymalCRoughStudentCfgPPO` (`anymal_c_rough_student_config.py`).  The gradient step is a plain restatement of
`rsl_rl/algorithms/distillation.py:107-153` in PyTorch for a feed-forward `StudentTeacher` (MSE behaviour cloning, one backward pass per
`gradient_length` = 15 batches, Adam 1e-3, grad clip 1.0 on the student); autograd stays in PyTorch.  The teacher is a checkpoint written by
`tools/train_acceptance.py --task anymal_c_rough` (`actor.*` fills the teacher, `student_teacher.py:125-138`); without one, a fixed random teacher.

`--python-loop`: the same iteration with the collection loop in Python -- `policy.act_and_teach` -> `env.step` (its torch history layer) -- the checker
of the native collector: with noise off the rows, and so the loss sequence, are equal.  `--eager-policy` (with `--python-loop`) also acts with the torch
modules instead of the native policy kernels.

`--update native`: the gradient step runs on the device too (`rl.NativeDistillation`, include/lgdistill.h); the `NativeStudentTeacher` is built once
and never rebuilt, and the saved checkpoint is the trainer's `state_dict()`.  The default, `torch`, is the eager update above.

`--student recurrent`: a `StudentTeacherRecurrent` (`--rnn-type` memory of `--rnn-hidden` units and `--rnn-layers` layers in front of the student
MLP; feed-forward teacher) collected by `lg_collect_distillation_recurrent`.  `--update torch` replays the rows through the torch memory as
`Distillation.update` does (truncated BPTT, dones applied, epochs seeded from the state the last update ended with, the clip on the MLP alone);
`--update native` is `rl.NativeRecurrentDistillation` (include/lgdistill_recurrent.h).  Either way the student memory continues from the end state of
the replay.  The default, `feedforward`, is everything above.

Training the registered task goes through `scripts/train.py --runner native` (`rl.NativeDistillationRunner`); this tool stays as the checker and the bench driver.

usage: python tools/train_distill.py [--teacher train_acceptance_model.pt] [--out distill.json] [--iters 100] [--envs 4096] [--python-loop]
                                     [--update {torch,native}] [--student {feedforward,recurrent}]
"""
import argparse
import ast
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mlp(dims):
    layers = []
    for i in range(len(dims) - 1):
        layers.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(torch.nn.ELU())
    return torch.nn.Sequential(*layers)


class StudentTeacher(torch.nn.Module):
    """The module tree of `rsl_rl/modules/student_teacher.py:15-73` (state-dict names `student.*`, `teacher.*`, `std`), feed-forward."""

    def __init__(self, num_student_obs, num_teacher_obs, num_actions, student_dims, teacher_dims, init_noise_std):
        super().__init__()
        self.student = mlp([num_student_obs] + list(student_dims) + [num_actions])
        self.teacher = mlp([num_teacher_obs] + list(teacher_dims) + [num_actions])
        self.teacher.eval()
        self.std = torch.nn.Parameter(init_noise_std * torch.ones(num_actions))

    def load_teacher(self, state_dict):
        """`StudentTeacher.load_state_dict` on a PPO checkpoint (`student_teacher.py:125-138`): `actor.*` -> the teacher."""
        self.teacher.load_state_dict({k.replace("actor.", ""): v for k, v in state_dict.items() if "actor." in k})


class _Memory(torch.nn.Module):
    def __init__(self, input_size, rnn_type, num_layers, hidden_size):
        super().__init__()
        self.rnn = (torch.nn.GRU if rnn_type == "gru" else torch.nn.LSTM)(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)


class StudentTeacherRecurrent(StudentTeacher):
    """The module tree of `rsl_rl/modules/student_teacher_recurrent.py:15-69` without a teacher memory: `memory_s.rnn.*` in front of the student."""

    def __init__(self, num_student_obs, num_teacher_obs, num_actions, student_dims, teacher_dims, init_noise_std, rnn_type="lstm", rnn_hidden=256, rnn_layers=1):
        super().__init__(rnn_hidden, num_teacher_obs, num_actions, student_dims, teacher_dims, init_noise_std)
        self.memory_s = _Memory(num_student_obs, rnn_type, rnn_layers, rnn_hidden)


def _map_state(state, fn):
    return None if state is None else (tuple(fn(s) for s in state) if isinstance(state, tuple) else fn(state))


def distill_update_recurrent(policy, optimizer, rows, carry, num_learning_epochs=1, gradient_length=15, max_grad_norm=1.0):
    """`Distillation.update` for a `StudentTeacherRecurrent`: every epoch enters with `carry` (the state the last update ended with, None: zeros);
    gradients flow through the memory inside a group only; after every step (and after the optimiser step's detach) the done rows are zeroed and
    nothing crosses.  Returns (mean behaviour loss, the new carry)."""
    obs, target, dones = rows["observations"], rows["privileged_actions"], rows["dones"]
    mean_loss, loss, cnt, state = 0.0, 0, 0, carry
    for _ in range(num_learning_epochs):
        state = carry
        for t in range(obs.shape[0]):
            out, state = policy.memory_s.rnn(obs[t].unsqueeze(0), state)
            behavior_loss = torch.nn.functional.mse_loss(policy.student(out.squeeze(0)), target[t])
            loss = loss + behavior_loss
            mean_loss += behavior_loss.item()
            cnt += 1
            if cnt % gradient_length == 0:
                optimizer.zero_grad()
                loss.backward()
                if max_grad_norm:
                    torch.nn.utils.clip_grad_norm_(policy.student.parameters(), max_grad_norm)
                optimizer.step()
                state = _map_state(state, lambda s: s.detach())
                loss = 0
            keep = (dones[t].view(1, -1, 1) == 0).to(out.dtype)
            state = _map_state(state, lambda s: s * keep)
    return mean_loss / cnt, _map_state(state, lambda s: s.detach())


def distill_update(policy, optimizer, rows, gradient_length=15, max_grad_norm=1.0):
    """`Distillation.update` (`distillation.py:107-153`), one epoch over the (T, N, .) rows in time order: returns the mean behaviour loss."""
    obs, target = rows["observations"], rows["privileged_actions"]
    mean_loss, loss, cnt = 0.0, 0, 0
    for t in range(obs.shape[0]):
        behavior_loss = torch.nn.functional.mse_loss(policy.student(obs[t]), target[t])
        loss = loss + behavior_loss
        mean_loss += behavior_loss.item()
        cnt += 1
        if cnt % gradient_length == 0:
            optimizer.zero_grad()
            loss.backward()
            if max_grad_norm:
                torch.nn.utils.clip_grad_norm_(policy.student.parameters(), max_grad_norm)
            optimizer.step()
            loss = 0
    return mean_loss / cnt


def collect_python_loop(env, native, num_steps, eager=None):
    """The loop `collect_distillation` replaces: Distillation.act -> env.step -> process_env_step (`distillation.py:89-105`), rows stacked (T, N, .)."""
    rows = {k: [] for k in ("observations", "privileged_observations", "actions", "privileged_actions", "rewards", "dones")}
    obs, priv = env.get_observations(), env.get_privileged_observations()
    for _ in range(num_steps):
        if eager is not None:
            with torch.no_grad():
                mean = eager.student(obs)
                actions, teach = torch.distributions.Normal(mean, eager.std.expand_as(mean)).sample(), eager.teacher(priv)
        else:
            actions, teach = native.act_and_teach(obs, priv)
        rows["observations"].append(obs.clone()); rows["privileged_observations"].append(priv.clone())
        rows["actions"].append(actions.clone()); rows["privileged_actions"].append(teach.clone())
        obs, priv, rew, dones, _ = env.step(actions)
        rows["rewards"].append(rew.clone().view(-1, 1)); rows["dones"].append(dones.float().view(-1, 1))
    return {k: torch.stack(v) for k, v in rows.items()}


def run(task="anymal_c_rough_student", envs=4096, iters=100, seed=1, teacher=None, python_loop=False, eager_policy=False, overrides=(), log=print,
        update="torch", student="feedforward", rnn_type="lstm", rnn_hidden=256, rnn_layers=1):
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.rl import (NativeDistillation, NativeRecurrentDistillation, NativeStudentTeacher, NativeStudentTeacherRecurrent,
                                            collect_distillation)
    from extended_legged_gym_amd.utils.helpers import class_to_dict, get_args
    torch.manual_seed(seed); np.random.seed(seed)
    env_cfg, train_cfg = task_registry.get_cfgs(task)
    env_cfg = copy.deepcopy(env_cfg)                 # (the registry's instance stays untouched)
    env_cfg.env.num_envs, env_cfg.seed = envs, seed
    for kv in overrides:
        key, val = kv.split("=", 1)
        obj, parts = env_cfg, key.split(".")
        for pth in parts[:-1]:
            obj = getattr(obj, pth)
        setattr(obj, parts[-1], ast.literal_eval(val))
    env, env_cfg = task_registry.make_env(task, args=get_args(["--headless", "--sim_device", "cuda:0"]), env_cfg=env_cfg)
    tc = class_to_dict(train_cfg)
    alg, pol, T = tc["algorithm"], tc["policy"], tc["runner"]["num_steps_per_env"]
    recurrent = student == "recurrent"
    if recurrent and (python_loop or eager_policy):
        raise ValueError("--student recurrent collects with the native collector only")
    shape = (env.num_obs, env.num_privileged_obs, env.num_actions, pol["student_hidden_dims"], pol["teacher_hidden_dims"], pol["init_noise_std"])
    policy = (StudentTeacherRecurrent(*shape, rnn_type, rnn_hidden, rnn_layers) if recurrent else StudentTeacher(*shape)).cuda()
    if teacher:
        policy.load_teacher(torch.load(teacher, map_location="cuda:0")["model_state_dict"])
    opt = torch.optim.Adam(policy.parameters(), lr=alg["learning_rate"])
    env.reset()
    losses = []
    if recurrent:
        E, kw = alg.get("num_learning_epochs", 1), dict(activation=pol["activation"], rnn_type=rnn_type, device="cuda:0", seed=seed)
        sd = {k: v.detach().clone() for k, v in policy.state_dict().items()}
        native = NativeStudentTeacherRecurrent(sd, **kw)          # --update native: built once, the trainer moves its student and memory in place
        trainer = carry = None
        if update == "native":
            trainer = NativeRecurrentDistillation(native, sd, num_learning_epochs=E, gradient_length=alg["gradient_length"], learning_rate=alg["learning_rate"],
                                                  max_grad_norm=alg["max_grad_norm"], loss_type=alg.get("loss_type", "mse"))
        for it in range(iters):
            if trainer is None and it > 0:          # rebuilt from the torch module's weights; its student memory continues from the end state of the replay
                native = NativeStudentTeacherRecurrent(policy.state_dict(), **kw)
                native._call = it * T
                native.reset(hidden_states=(carry, None))
            rows = collect_distillation(env, native, T)
            if trainer is not None:
                losses.append(trainer.update(rows)["behavior"])
            else:
                loss, carry = distill_update_recurrent(policy, opt, rows, carry, E, alg["gradient_length"], alg["max_grad_norm"])
                losses.append(loss)
            log(f"iteration {it}: behaviour loss {losses[-1]:.9g}  mean reward {float(rows['rewards'].mean()):.5f}  dones {int(rows['dones'].sum())}")
        if trainer is not None:
            policy.load_state_dict({k: v.to("cuda:0") for k, v in trainer.state_dict().items()})
        return losses, policy
    if update == "native":
        if eager_policy:
            raise ValueError("--eager-policy acts with the torch modules, which --update native never refreshes")
        sd = {k: v.detach().clone() for k, v in policy.state_dict().items()}
        native = NativeStudentTeacher(sd, activation=pol["activation"], device="cuda:0", seed=seed)          # built once: the trainer moves its student in place
        trainer = NativeDistillation(native, sd, num_learning_epochs=alg.get("num_learning_epochs", 1), gradient_length=alg["gradient_length"],
                                     learning_rate=alg["learning_rate"], max_grad_norm=alg["max_grad_norm"], loss_type=alg.get("loss_type", "mse"))
        for it in range(iters):
            rows = collect_python_loop(env, native, T) if python_loop else collect_distillation(env, native, T)
            losses.append(trainer.update(rows)["behavior"])
            log(f"iteration {it}: behaviour loss {losses[-1]:.9g}  mean reward {float(rows['rewards'].mean()):.5f}  dones {int(rows['dones'].sum())}")
        policy.load_state_dict({k: v.to("cuda:0") for k, v in trainer.state_dict().items()})          # the checkpoint: the trainer's state dict
        return losses, policy
    for it in range(iters):
        # the native policy is rebuilt from the torch module's weights after every update (tools/train_acceptance.py does the same for PPO)
        native = NativeStudentTeacher(policy.state_dict(), activation=pol["activation"], device="cuda:0", seed=seed)
        native._call = it * T
        if python_loop:
            rows = collect_python_loop(env, native, T, policy if eager_policy else None)
        else:
            rows = collect_distillation(env, native, T)
        losses.append(distill_update(policy, opt, rows, alg["gradient_length"], alg["max_grad_norm"]))
        log(f"iteration {it}: behaviour loss {losses[-1]:.9g}  mean reward {float(rows['rewards'].mean()):.5f}  dones {int(rows['dones'].sum())}")
    return losses, policy


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="anymal_c_rough_student")
    ap.add_argument("--teacher", default=None, help="checkpoint of tools/train_acceptance.py (default: a fixed random teacher)")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--python-loop", action="store_true", help="collect with env.step from Python (the checker of the native collector)")
    ap.add_argument("--eager-policy", action="store_true", help="with --python-loop: act with the torch modules, not the native policy kernels")
    ap.add_argument("--set", action="append", default=[], metavar="section.key=value", help="override of the task's env config, e.g. noise.add_noise=False")
    ap.add_argument("--update", choices=("torch", "native"), default="torch", help="the gradient step: eager PyTorch, or rl.NativeDistillation on the device")
    ap.add_argument("--student", choices=("feedforward", "recurrent"), default="feedforward", help="recurrent: a StudentTeacherRecurrent (memory in front of the student)")
    ap.add_argument("--rnn-type", choices=("lstm", "gru"), default="lstm")
    ap.add_argument("--rnn-hidden", type=int, default=256)
    ap.add_argument("--rnn-layers", type=int, default=1)
    ap.add_argument("--out", default=None, help="write the loss curve here (JSON) and the trained modules next to it (_model.pt)")
    a = ap.parse_args(argv)
    losses, policy = run(a.task, a.envs, a.iters, a.seed, a.teacher, a.python_loop, a.eager_policy, a.set, update=a.update, student=a.student,
                         rnn_type=a.rnn_type, rnn_hidden=a.rnn_hidden, rnn_layers=a.rnn_layers)
    if not a.out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"task": a.task, "envs": a.envs, "python_loop": a.python_loop, "update": a.update, "student": a.student, "behaviour_loss": losses}, f)
    torch.save({"model_state_dict": policy.state_dict(), "iter": a.iters}, os.path.splitext(a.out)[0] + "_model.pt")


if __name__ == "__main__":
    main()
