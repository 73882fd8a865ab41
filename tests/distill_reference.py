"""A torch restatement of `Distillation.update` of the vendored rsl_rl (`algorithms/distillation.py:107-153`, batches in time order as
`storage/rollout_storage.py:170-182`) for the feed-forward `StudentTeacher`: the sequence of E * T steps, every `gradient_length` consecutive ones
(across the epoch boundary) one optimiser step on the gradient of the SUM of their mean losses, the trailing steps evaluated with the final weights
and never trained on, the clip skipped for a `max_grad_norm` of None or 0, Adam on the student alone.  dtype-generic like tests/ppo_reference.py,
whose `mlp`, `cast` and `clip_and_adam` it reuses: float64 is the reference the native update is held to, float32 sets the bar.
tests/test_distill_update_reference.py holds this file to the reference's own update (tests/golden/distillation_update.npz)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.ppo_reference import cast, clip_and_adam, fresh_state, layer_names, mlp

LOSSES = {"mse": F.mse_loss, "huber": F.huber_loss}          # huber: delta = 1, torch's default


def student_of(sd):
    return {k: v for k, v in sd.items() if k.startswith("student.")}


def group_gradients(sd, act, obs, target, first_step, num_steps, loss_type="mse", dtype=torch.float64):
    """One group: step s reads time index (first_step + s) mod T.  Returns (gradients of the student's tensors before the clip, global norm, the
    per-step losses, the per-step differences d = student action - target)."""
    p = {k: v.requires_grad_(True) for k, v in cast(student_of(sd), dtype).items()}
    obs, target = obs.to(dtype), target.to(dtype)
    T = obs.shape[0]
    total, losses, diffs = 0, [], []
    for s in range(num_steps):
        t = (first_step + s) % T
        out = mlp(p, "student", obs[t], act)
        loss = LOSSES[loss_type](out, target[t])
        total = total + loss
        losses.append(loss.detach())
        diffs.append((out - target[t]).detach())
    total.backward()
    grads = {k: v.grad.detach() for k, v in p.items()}
    norm = torch.sqrt(sum((g ** 2).sum() for g in grads.values()))
    return grads, norm, losses, diffs


def step_loss(sd, act, obs_t, target_t, loss_type, dtype):
    with torch.no_grad():
        out = mlp(cast(student_of(sd), dtype), "student", obs_t.to(dtype), act)
        return LOSSES[loss_type](out, target_t.to(dtype)), out - target_t.to(dtype)


def update(sd, act, obs, target, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse",
           dtype=torch.float64, state=None):
    """The whole update.  Returns (state dict: student.* updated, the rest as given; {"behavior": mean}; trace), trace: the step losses (Python
    floats, summed as the reference sums `.item()`s), per group the norm and the differences d, the differences of the remainder steps, and the
    optimiser state."""
    params = cast(student_of(sd), dtype)
    state = state if state is not None else fresh_state(params, dtype)
    T = obs.shape[0]
    total, k = num_learning_epochs * T, 0
    losses, norms, group_diffs = [], [], []
    while total - k >= gradient_length:
        grads, norm, ls, ds = group_gradients(params, act, obs, target, k, gradient_length, loss_type, dtype)
        params, state = clip_and_adam(params, grads, state, learning_rate, max_grad_norm if max_grad_norm else float("inf"), dtype)
        losses += [float(x) for x in ls]
        norms.append(float(norm))
        group_diffs.append(torch.stack(ds))
        k += gradient_length
    rest = []
    for j in range(k, total):
        loss, d = step_loss(params, act, obs[j % T], target[j % T], loss_type, dtype)
        losses.append(float(loss))
        rest.append(d)
    out = {k2: v.clone() for k2, v in sd.items()}
    out.update(params)
    return out, {"behavior": sum(losses) / total}, dict(step_losses=losses, norms=norms, group_diffs=group_diffs, rest_diffs=rest, state=state)


def craft_rows(sd, act, T, N, seed, spread=1.0):
    """Seeded float32 observations (T, N, S) and targets (T, N, A) around the CURRENT student: target = student action - d with d = spread * N(0, 1),
    so that at spread 1 about a third of the elements sit on the linear side of the Huber loss; an element within 1e-3 of the kink |d| = 1 is
    moved 1 % outwards."""
    g = torch.Generator().manual_seed(seed)
    p = cast(student_of(sd), torch.float32)
    S = p[f"student.{layer_names(p, 'student')[0]}.weight"].shape[1]
    obs = torch.randn(T, N, S, generator=g)
    with torch.no_grad():
        out = mlp(p, "student", obs, act)
    d = spread * torch.randn(out.shape, generator=g)
    d = torch.where(((d.abs() - 1.0).abs() < 1e-3), d * 1.01, d)
    return dict(observations=obs, privileged_actions=(out - d).contiguous())


def huber_fractions(d):
    """(fraction of elements with |d| > 1, with |d| < 1, the smallest ||d| - 1|)."""
    a = d.double().abs()
    return float((a > 1).double().mean()), float((a < 1).double().mean()), float((a - 1).abs().min())


def random_student(dims, seed, teacher_dims=None, std=0.5):
    """A `StudentTeacher` state dict with a random student (and a small teacher, which no update may touch)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for prefix, ds in (("student", dims), ("teacher", teacher_dims or [dims[0] + 3, 8, dims[-1]])):
        for j in range(len(ds) - 1):
            bound = 1.0 / np.sqrt(ds[j])
            sd[f"{prefix}.{2 * j}.weight"] = (torch.rand(ds[j + 1], ds[j], generator=g) * 2 - 1) * bound * 1.7
            sd[f"{prefix}.{2 * j}.bias"] = (torch.rand(ds[j + 1], generator=g) * 2 - 1) * bound
    sd["std"] = std * torch.ones(dims[-1])
    return sd


# The shapes of tests/test_hip_distill_update.py: (student widths, activation, N, G).  D2's N makes G * N two full weight-gradient slabs and a
# ragged third of 13 rows, with a time-step boundary inside a slab.
def shape_case(shape, slab_rows):
    if shape == "D1":
        return random_student([13, 20, 9, 5], 21), "tanh", 37, 3
    if shape.startswith("D2"):
        assert (2 * slab_rows + 13) % 3 == 0, slab_rows
        return random_student([48, 64, 32, 12], 22), shape.split("-")[1], (2 * slab_rows + 13) // 3, 3
    if shape == "D3":
        return random_student([5, 3], 23), "elu", 37, 2
    if shape == "D4":
        return random_student([144, 512, 256, 128, 12], 24), "elu", 32, 3
    raise KeyError(shape)


SHAPES = ("D1", "D2-elu", "D2-relu", "D2-selu", "D3", "D4")
GROUP_SEED = 31          # craft_rows seed of the one-group checks
# the optimiser-step check (D1, mse): rows this far from the student put the group's norm well above 1, between the clip that bites and the one that does not
OPT_SPREAD, CLIP_SMALL, CLIP_LARGE = 4.0, 0.05, 1.0e3


def load_golden_case(name):
    """A case of tests/golden/distillation_update.npz (tools/refgen/make_distillation_update_golden.py): the state dict before (`sd0`, stored as
    float16, exact) and after (`sd1`) the reference's `Distillation.update`, the storage rows, the returned loss and the settings."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distillation_update.npz"))
    part = lambda tag: {k[len(name) + len(tag) + 2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith(f"{name}.{tag}.")}  # noqa: E731
    cfg = json.loads(str(z[f"{name}.config"]))
    return dict(sd0=part("sd0"), sd1=part("sd1"), observations=torch.from_numpy(z[f"{name}.observations"]),
                privileged_actions=torch.from_numpy(z[f"{name}.privileged_actions"]), dones=torch.from_numpy(z[f"{name}.dones"]),
                loss=float(z[f"{name}.loss"]), **cfg)
