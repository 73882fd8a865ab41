"""Native distillation update of the recurrent student (rl.NativeRecurrentDistillation, include/lgdistill_recurrent.h) against the eager-torch
`distill_update_recurrent` of tools/train_distill.py, interleaved in one process, on the same recorded rows.

Workload: `anymal_c_rough_student`'s 144-wide history rows through an LSTM of 256 units (one layer) and the registered student MLP
(256-512-256-128-12, ELU), 4096 envs x 24 steps collected once by `collect_distillation` from a fixed random teacher, gradient_length 15, one epoch:
one optimiser step over 15 steps x 4096 rows (truncated BPTT through 15 steps) and nine forward-only steps.  Per side: `--warmup` updates, then
`--reps` timed ones, the two sides alternating; wall clock around a device synchronisation (the native update is one enqueue and one device-to-host
copy; the torch side synchronises at every `.item()` by itself).  Both sides start every timed update from their own carried state.

usage: python tools/bench_distillation_recurrent_update.py [--reps 5] [--warmup 2] [--out profiles/distillation_recurrent_update.json]"""
import argparse
import copy
import datetime
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def library_hash():
    with open(os.path.join(ROOT, "extended_legged_gym_amd", "csrc", "liblgstep.so"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rnn-type", choices=("lstm", "gru"), default="lstm")
    ap.add_argument("--rnn-hidden", type=int, default=256)
    ap.add_argument("--rnn-layers", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distillation_recurrent_update.json"))
    a = ap.parse_args(argv)
    import train_distill
    from extended_legged_gym_amd.envs import task_registry
    from extended_legged_gym_amd.rl import NativeRecurrentDistillation, NativeStudentTeacherRecurrent, collect_distillation
    from extended_legged_gym_amd.utils.helpers import class_to_dict, get_args
    task, G, E = "anymal_c_rough_student", 15, 1
    torch.manual_seed(1)
    env_cfg, train_cfg = task_registry.get_cfgs(task)
    env_cfg = copy.deepcopy(env_cfg)
    env_cfg.env.num_envs, env_cfg.seed = a.envs, 1
    env, _ = task_registry.make_env(task, args=get_args(["--headless", "--sim_device", "cuda:0"]), env_cfg=env_cfg)
    tc = class_to_dict(train_cfg)
    pol, T = tc["policy"], tc["runner"]["num_steps_per_env"]
    module = train_distill.StudentTeacherRecurrent(env.num_obs, env.num_privileged_obs, env.num_actions, pol["student_hidden_dims"], pol["teacher_hidden_dims"],
                                                   pol["init_noise_std"], a.rnn_type, a.rnn_hidden, a.rnn_layers).cuda()
    opt = torch.optim.Adam(module.parameters(), lr=1e-3)
    sd = {k: v.detach().clone() for k, v in module.state_dict().items()}
    native = NativeStudentTeacherRecurrent(sd, activation=pol["activation"], rnn_type=a.rnn_type, device="cuda:0", seed=1)
    trainer = NativeRecurrentDistillation(native, sd, num_learning_epochs=E, gradient_length=G, learning_rate=1e-3, max_grad_norm=1.0)
    env.reset()
    rows = collect_distillation(env, native, T)          # recorded once; both sides train on these
    torch.cuda.synchronize()
    times, losses, carry = {"native": [], "torch": []}, {"native": [], "torch": []}, None
    for rep in range(a.warmup + a.reps):
        for side in ("native", "torch"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if side == "native":
                loss = trainer.update(rows)["behavior"]
            else:
                loss, carry = train_distill.distill_update_recurrent(module, opt, rows, carry, E, G, 1.0)
            torch.cuda.synchronize()
            if rep >= a.warmup:
                times[side].append((time.perf_counter() - t0) * 1e3)
            losses[side].append(loss)
    result = dict(device=torch.cuda.get_device_name(0), date=datetime.date.today().isoformat(), library_sha256=library_hash(), task=task,
                  memory=dict(type=a.rnn_type, input=env.num_obs, hidden=a.rnn_hidden, layers=a.rnn_layers),
                  student=[a.rnn_hidden] + list(pol["student_hidden_dims"]) + [env.num_actions], activation=pol["activation"], envs=a.envs, steps=T, gradient_length=G,
                  epochs=E, optimizer_steps_per_update=(E * T) // G, rows_per_optimizer_step=G * a.envs, warmup=a.warmup, workspace_bytes=trainer.workspace_bytes())
    for side, ts in times.items():
        result[side] = dict(ms_per_update_median=statistics.median(ts), ms_per_update_min=min(ts), ms_per_update_max=max(ts), reps=len(ts), losses=losses[side])
    result["native_over_torch"] = result["native"]["ms_per_update_median"] / result["torch"]["ms_per_update_median"]
    print(json.dumps({k: v for k, v in result.items() if k not in ("native", "torch")}), flush=True)
    print("native", result["native"], "\ntorch", result["torch"], flush=True)
    trainer.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
