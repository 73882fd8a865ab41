"""Golden vectors for the native distillation update of the recurrent student: the reference's vendored rsl_rl (`Distillation`,
`RolloutStorage("distillation", ...)`, `StudentTeacherRecurrent`) run in the build container on torch-CPU, in the style of
make_distillation_update_golden.py (fp16-representable parameters, seeded rows).  Per case TWO successive rounds of collecting T steps through
`Distillation.act` / `process_env_step` and `Distillation.update`, so that the second update starts from a non-zero carry; each in fp32 and in float64.

  lstm                    LSTM student memory, feed-forward teacher
  gru_teacher_recurrent   GRU memories in front of student and teacher

Sizes (tests/distill_recurrent_reference.GOLDEN): student obs 20, hidden 24 (40 would put the four recorded state dicts of a case past the size a
committed file may have), 2 memory layers, MLP [32, 16], 12 actions, 7 rows, T 7, G 3, E 2, huber, lr 2e-3; dones at a group's first step, at a group's
last step and at t = T - 1 (UPDATE_DONES).  max_grad_norm is CLIP_SMALL, below every recorded `student.*` norm (asserted here), so the clip bites in every
optimiser step.

Recorded per case: sd0 (float16), per round r and precision p (f32 | f64): observations, teacher_observations, privileged_actions, dones, the E * T
step losses, the returned mean, the norms `clip_grad_norm_` saw, `student.*` and `memory_s.*` after the update (everything else is asserted
unchanged here), `last_hidden_states` (the carry) and `policy.get_hidden_states()` after the update (student: h, c; teacher: present or not).  Data only."""
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
from rsl_rl.modules import StudentTeacherRecurrent  # noqa: E402
from tests import distill_recurrent_reference as ref  # noqa: E402

TEACHER_OBS = 17


def parts(prefix, state, out):
    """h | (h, c) | None under prefix.h / prefix.c; prefix.present says whether there was a state."""
    out[prefix + ".present"] = np.int64(state is not None)
    if state is not None:
        for k, v in ref.state_parts(state).items():
            out[f"{prefix}.{k}"] = v.detach().numpy().copy()


def run(name, cfg, sd0, inputs, dtype, out):
    G = ref.GOLDEN
    tag = "f32" if dtype == torch.float32 else "f64"
    torch.set_default_dtype(dtype)
    try:
        torch.manual_seed(0)
        policy = StudentTeacherRecurrent(G["S"], TEACHER_OBS, G["A"], student_hidden_dims=list(G["mlp"]), teacher_hidden_dims=[24], activation="elu",
                                         rnn_type=cfg["rnn"], rnn_hidden_dim=G["H"], rnn_num_layers=G["layers"], teacher_recurrent=cfg["teacher_recurrent"])
        policy.load_state_dict({k: v.to(dtype) for k, v in sd0.items()})
        policy.loaded_teacher = True
        algo = Distillation(policy, num_learning_epochs=G["E"], gradient_length=G["G"], learning_rate=G["lr"], max_grad_norm=ref.CLIP_SMALL, loss_type=G["loss"],
                            device="cpu")
        algo.init_storage("distillation", G["N"], G["T"], [G["S"]], [TEACHER_OBS], [G["A"]])
        losses, norms = [], []
        fn = algo.loss_fn

        def recording_loss(a, b):
            l = fn(a, b)
            losses.append(l.item())
            return l
        algo.loss_fn = recording_loss
        clip = torch.nn.utils.clip_grad_norm_

        def recording_clip(params, max_norm):
            n = clip(params, max_norm)
            norms.append(float(n))
            return n
        torch.nn.utils.clip_grad_norm_ = recording_clip
        try:
            for r, (obs, tobs, dones) in enumerate(inputs):
                losses.clear(); norms.clear()
                for t in range(G["T"]):
                    algo.act(obs[t].to(dtype), tobs[t].to(dtype))
                    algo.process_env_step(torch.zeros(G["N"], dtype=dtype), dones[t], {})
                targets = algo.storage.privileged_actions.detach().clone()
                mean = algo.update()["behavior"]
                assert len(losses) == G["E"] * G["T"] and len(norms) == (G["E"] * G["T"]) // G["G"]
                assert min(norms) > ref.CLIP_SMALL, (name, tag, r, norms)          # the clip bites in every optimiser step
                p = f"{name}.r{r}.{tag}"
                out[p + ".privileged_actions"] = targets.numpy().copy()
                out[p + ".step_losses"] = np.array(losses, np.float64)
                out[p + ".loss"] = np.float64(mean)
                out[p + ".norms"] = np.array(norms, np.float64)
                for k, v in policy.state_dict().items():
                    if k.startswith("student.") or k.startswith("memory_s."):
                        out[f"{p}.sd.{k}"] = v.detach().numpy().copy()
                    else:
                        assert torch.equal(v, sd0[k].to(dtype)), k          # the teacher, its memory and std never move
                parts(p + ".carry", algo.last_hidden_states[0], out)
                hs = policy.get_hidden_states()
                parts(p + ".hidden_s", hs[0], out)
                parts(p + ".hidden_t", hs[1], out)
                print(name, tag, "round", r, "loss", mean, "norms", norms)
        finally:
            torch.nn.utils.clip_grad_norm_ = clip
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    out, G = {}, ref.GOLDEN
    for i, (name, cfg) in enumerate(ref.GOLDEN_CASES.items()):
        torch.manual_seed(100 + i)
        policy = StudentTeacherRecurrent(G["S"], TEACHER_OBS, G["A"], student_hidden_dims=list(G["mlp"]), teacher_hidden_dims=[24], activation="elu",
                                         rnn_type=cfg["rnn"], rnn_hidden_dim=G["H"], rnn_num_layers=G["layers"], teacher_recurrent=cfg["teacher_recurrent"])
        g = torch.Generator().manual_seed(300 + i)
        sd0 = {}
        for k, v in policy.state_dict().items():          # the memories a little wider than torch's default, so that gradients through time carry weight
            scale = 1.5 if "memory" in k and v.dim() == 2 else 1.0
            sd0[k] = (scale * v).to(torch.float16).to(torch.float32)
        inputs = []
        for r in range(G["rounds"]):
            obs = torch.randn(G["T"], G["N"], G["S"], generator=g)
            tobs = 1.5 * torch.randn(G["T"], G["N"], TEACHER_OBS, generator=g)
            dones = torch.zeros(G["T"], G["N"])
            for t, rows in ref.UPDATE_DONES.items():
                dones[t, [(j + r) % G["N"] for j in rows]] = 1.0
            inputs.append((obs, tobs, dones))
            out[f"{name}.r{r}.observations"] = obs.numpy()
            out[f"{name}.r{r}.teacher_observations"] = tobs.numpy()
            out[f"{name}.r{r}.dones"] = dones.numpy()
        for k, v in sd0.items():
            out[f"{name}.sd0.{k}"] = v.numpy().astype(np.float16)
        out[f"{name}.config"] = np.array(json.dumps(dict(activation="elu", teacher_obs=TEACHER_OBS, max_grad_norm=ref.CLIP_SMALL, **cfg, **{k: v for k, v in G.items()})))
        for dtype in (torch.float32, torch.float64):
            run(name, cfg, sd0, inputs, dtype, out)
    path = ref.GOLDEN_FILE
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
