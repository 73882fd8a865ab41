"""A torch-CPU restatement of `Distillation.update` for the recurrent student (`rsl_rl/algorithms/distillation.py:107-153` with
`modules/student_teacher_recurrent.py:71-100` and `networks/memory.py:35-65`, as include/lgdistill_recurrent.h restates it) for the tests of
`rl.NativeRecurrentDistillation`: group gradients and whole updates by autograd over an `nn.LSTM` / `nn.GRU` in front of an `nn.Sequential`, in
float64 (the reference) and in float32 (torch's own rounding, which sets the bar).  No rsl_rl import; no test here.

The semantics restated: E * T steps epoch-major; every G consecutive steps one optimiser step on the sum of their losses; the trailing steps forward
only.  Gradients flow through the memory inside a group only.  After every step the rows with dones != 0 are zeroed in every layer and nothing
crosses; at a step that ends a group the order is optimiser step, detach, zero.  A step with time index 0 enters with the carry (the state the last
update ended with; zeros before the first), not with the previous epoch's end.  The clip's norm is taken over `student.*` alone and its scale is
applied to `student.*` alone; Adam (torch's defaults) runs over `student.*` + `memory_s.*`.

Weights and rows are seeded; the weights are float16-exact, as in the goldens.

The optional `faults` break the restatement in the ways an implementation can go wrong; tests/test_distill_recurrent_update_reference.py shows that
the bar of the GPU test sees each of them (its power):
  cross_done        the zeroing of a done row lets the gradient through (forward zero, backward identity)
  no_detach         `group_gradients(pre_steps=...)`: the chain is not cut at the group's first step (gradient crossing a group boundary)
  epoch_chain       an epoch starts from the previous epoch's end instead of the carry
  clip_all          the clip's norm is taken over all trained parameters (and its scale applied to all)
  clip_memory       the clip's norm is student.*'s, but its scale is applied to memory_s.* too
  dones_before_detach  at a step that ends a group, the rows are zeroed in the tensor the detach then replaces from the saved state: the zeroing of
                    that step is lost
  whh_first_step    the weight_hh gradient of the upper memory layer misses the group's first step"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

MEMORY_NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
ACTS = {"elu": nn.ELU, "relu": nn.ReLU, "tanh": nn.Tanh}


class _Memory(nn.Module):
    def __init__(self, S, H, layers, rnn):
        super().__init__()
        self.rnn = (nn.GRU if rnn == "gru" else nn.LSTM)(input_size=S, hidden_size=H, num_layers=layers)


class StudentRecurrentTorch(nn.Module):
    """The trained part of a `StudentTeacherRecurrent`, with its state-dict names: `student.{0,2,..}`, `memory_s.rnn.*`."""

    def __init__(self, S, H, layers, mlp, A, rnn="lstm", act="elu"):
        super().__init__()
        dims, mods = [H, *mlp, A], []
        for i in range(len(dims) - 1):
            mods.append(nn.Linear(dims[i], dims[i + 1]))
            if i < len(dims) - 2:
                mods.append(ACTS[act]())
        self.student = nn.Sequential(*mods)
        self.memory_s = _Memory(S, H, layers, rnn)


class Case:
    """One student and its rows.  S observations, hidden H, `layers` memory layers, MLP hidden widths `mlp`, A actions; N envs, T steps; G: the
    group length the tests use.  dones_at: {time index: rows} (rows None: every other row, alternating with t)."""

    def __init__(self, name, S=20, H=40, layers=2, mlp=(32, 16), A=12, N=7, G=3, T=None, rnn="lstm", act="elu", loss="huber", salt=0, dones_at=None):
        self.name, self.S, self.H, self.layers, self.mlp, self.A, self.N, self.G, self.T = name, S, H, layers, tuple(mlp), A, N, G, T or G
        self.rnn, self.act, self.loss, self.salt, self.dones_at = rnn, act, loss, salt, dict(dones_at or {})

    def state(self):
        """Seeded float16-exact parameters, fp32, in the flat order (student.*, then memory_s.*)."""
        m = StudentRecurrentTorch(self.S, self.H, self.layers, self.mlp, self.A, self.rnn, self.act)
        g = torch.Generator().manual_seed(4321 + self.salt)
        out = {}
        for k, v in m.state_dict().items():
            fan = v.shape[1] if v.dim() == 2 else v.shape[0]
            scale = (1.5 if k.startswith("memory_s") else 1.0) / fan ** 0.5 if v.dim() == 2 else 0.1
            out[k] = (scale * torch.randn(v.shape, generator=g)).half().float()
        return out

    def module(self, dtype=torch.float32, state=None):
        m = StudentRecurrentTorch(self.S, self.H, self.layers, self.mlp, self.A, self.rnn, self.act)
        m.load_state_dict(state if state is not None else self.state())
        return m.to(dtype)

    def rows(self, salt=0):
        """observations (T, N, S), privileged_actions (T, N, A), dones (T, N): fp32.  Targets spread so that |diff| lies on both sides of 1 (the
        Huber kink)."""
        T, N = self.T, self.N
        g = torch.Generator().manual_seed(1234 + self.salt + 1000 * salt)
        obs = torch.randn(T, N, self.S, generator=g)
        tgt = 1.2 * torch.randn(T, N, self.A, generator=g)
        dones = torch.zeros(T, N)
        for t, rows in self.dones_at.items():
            if rows is None:
                dones[t, (torch.arange(N) + t) % 2 == 0] = 1.0
            else:
                dones[t, list(rows)] = 1.0
        return dict(observations=obs, privileged_actions=tgt, dones=dones)


def carry_of(case, seed=77):
    """A seeded non-zero state to enter with: h, or (h, c)."""
    g = torch.Generator().manual_seed(seed + case.salt)
    h = 0.5 * torch.randn(case.layers, case.N, case.H, generator=g)
    return (h, 0.5 * torch.randn(case.layers, case.N, case.H, generator=g)) if case.rnn == "lstm" else h


def loss_fn(name):
    return {"mse": F.mse_loss, "huber": F.huber_loss}[name]


def zero_state(case, dtype):
    h = torch.zeros(case.layers, case.N, case.H, dtype=dtype)
    return (h, h.clone()) if case.rnn == "lstm" else h


def _each(state):
    return state if isinstance(state, tuple) else (state,)


def _like(state, parts):
    parts = tuple(parts)
    return parts if isinstance(state, tuple) else parts[0]


def detach(state):
    return _like(state, (s.detach() for s in _each(state)))


def cast(state, dtype):
    return _like(state, (s.detach().to(dtype).clone() for s in _each(state)))


class _LeakyMask(torch.autograd.Function):
    """The fault `cross_done`: zero forward, identity backward."""

    @staticmethod
    def forward(ctx, s, keep):
        return s * keep

    @staticmethod
    def backward(ctx, d):
        return d, None


def mask(state, dones, faults=None):
    """`Memory.reset(dones)` + `detach_hidden_states(dones)`: the rows with dones != 0 get zero state; no gradient crosses."""
    keep = (dones == 0).to(_each(state)[0].dtype).view(1, -1, 1)
    if faults and faults.get("cross_done"):
        return _like(state, (_LeakyMask.apply(s, keep) for s in _each(state)))
    return _like(state, (s * keep for s in _each(state)))


def step(model, rows, t, state, swap=None):
    """One step of every row at time index t from `state`: (actions, new state).  swap: {name: tensor} stands in for the memory's parameters of
    that name in this step only."""
    rnn, x = model.memory_s.rnn, rows["observations"][t].unsqueeze(0)
    if swap:
        out, state = torch.func.functional_call(rnn, {**dict(rnn.named_parameters()), **swap}, (x, state))
    else:
        out, state = rnn(x, state)
    return model.student(out.squeeze(0)), state


def to_dtype(rows, dtype):
    return {k: v.to(dtype) for k, v in rows.items()}


def student_parameters(model):
    return list(model.student.parameters())


def norm_of(params):
    return torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params)).item()


def named_grads(model):
    """The gradients in the state dict's names."""
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def group_gradients(case, dtype=torch.float64, first_step=0, num_steps=None, enter=None, carry=None, faults=None, state=None, pre_steps=0, rows=None):
    """The gradient of the SUM of the losses of steps [first_step, first_step + num_steps): (grads by name, (student norm, memory norm), step
    losses, actions (steps, N, A), the state after the last step with its dones applied).  enter: the state the first step enters with when its
    time index is not 0 (zeros if None); carry: the state a step with time index 0 enters with (zeros if None).  pre_steps: that many steps
    before first_step are run first, with the same weights and without a loss, to produce the entering state -- as a constant, unless the fault
    `no_detach` leaves the chain uncut at the group's first step."""
    faults = faults or {}
    model = case.module(dtype, state)
    rows, fn = to_dtype(rows if rows is not None else case.rows(), dtype), loss_fn(case.loss)
    nsteps = case.G if num_steps is None else num_steps
    st = cast(enter, dtype) if enter is not None else zero_state(case, dtype)
    for s in range(-pre_steps, 0):
        t = (first_step + s) % case.T
        if t == 0:
            st = cast(carry, dtype) if carry is not None else zero_state(case, dtype)
        st = mask(step(model, rows, t, st)[1], rows["dones"][t])
    if pre_steps and not faults.get("no_detach"):
        st = detach(st)
    total, losses, acts, shadow = 0, [], [], None
    for s in range(nsteps):
        t = (first_step + s) % case.T
        if t == 0:
            st = cast(carry, dtype) if carry is not None else zero_state(case, dtype)
        swap = None
        if s == 0 and faults.get("whh_first_step"):           # the first step's use of the upper layer's weight_hh collects its gradient elsewhere
            name = f"weight_hh_l{case.layers - 1}"
            shadow = getattr(model.memory_s.rnn, name).detach().clone().requires_grad_()
            swap = {name: shadow}
        a, st = step(model, rows, t, st, swap)
        l = fn(a, rows["privileged_actions"][t])
        total = total + l
        losses.append(l.item()); acts.append(a.detach())
        st = mask(st, rows["dones"][t], faults)
    model.zero_grad()
    total.backward()
    mem = list(model.memory_s.parameters())
    return named_grads(model), (norm_of(student_parameters(model)), norm_of(mem)), losses, torch.stack(acts), detach(st)


def clip_student(model, max_grad_norm, faults=None):
    """`nn.utils.clip_grad_norm_(policy.student.parameters(), max_grad_norm)`; returns the norm the clip used."""
    faults = faults or {}
    student, everything = student_parameters(model), list(model.parameters())
    if faults.get("clip_all"):
        return float(nn.utils.clip_grad_norm_(everything, max_grad_norm))
    norm = float(nn.utils.clip_grad_norm_(student, max_grad_norm))
    if faults.get("clip_memory"):
        coef = min(1.0, max_grad_norm / (norm + 1e-6))
        for p in model.memory_s.parameters():
            p.grad.mul_(coef)
    return norm


def student_clip_and_adam(params, grads, state, lr, max_grad_norm, dtype=torch.float64, faults=None):
    """One optimiser step out of place (`clip_and_adam` of tests/ppo_reference.py) with the clip rule of the recurrent student: the norm over
    `student.*`, the scale on `student.*`; `memory_s.*` enters Adam unscaled.  Returns (parameters, state, the norm the clip used)."""
    from tests import ppo_reference as pref
    faults = faults or {}
    g = {k: v.to(dtype) for k, v in grads.items()}
    student = [k for k in g if k.startswith("student.")]
    norm = torch.sqrt(sum((g[k] ** 2).sum() for k in (g if faults.get("clip_all") else student)))
    coef = min(1.0, max_grad_norm / (float(norm) + 1e-6)) if max_grad_norm else 1.0
    scaled = {k: v * coef if (k in student or faults.get("clip_all") or faults.get("clip_memory")) else v for k, v in g.items()}
    new_p, new_state = pref.clip_and_adam(params, scaled, state, lr, float("inf"), dtype)
    return new_p, new_state, float(norm)


def run_update(case, dtype=torch.float64, E=1, G=None, lr=1e-3, max_grad_norm=None, carry=None, model=None, optimizer=None, faults=None, rows=None,
               record_norms=False):
    """A whole update.  Returns dict: model, optimizer, losses (E T), mean, grad_norm / memory_grad_norm (of the last optimiser step before the
    clip, None if none), carry, steps; record_norms: norms, what `clip_grad_norm_` returned per optimiser step.  rows: other rows than the case's
    own (same shapes)."""
    faults = faults or {}
    G = G or case.G
    if model is None:
        model = case.module(dtype)
        optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    rows, fn = to_dtype(rows if rows is not None else case.rows(), dtype), loss_fn(case.loss)
    T = case.T
    carry0 = cast(carry, dtype) if carry is not None else zero_state(case, dtype)
    st, total, losses, cnt, norm, mnorm, steps, norms = carry0, 0, [], 0, None, None, 0, []
    for k in range(E * T):
        t = k % T
        if t == 0 and not (faults.get("epoch_chain") and k > 0):
            st = carry0
        a, st = step(model, rows, t, st)
        l = fn(a, rows["privileged_actions"][t])
        total = total + l
        losses.append(l.item())
        cnt += 1
        stepped = cnt % G == 0
        if stepped:
            optimizer.zero_grad()
            total.backward()
            norm, mnorm = norm_of(student_parameters(model)), norm_of(list(model.memory_s.parameters()))
            if max_grad_norm:
                used = clip_student(model, max_grad_norm, faults)
                if record_norms:
                    norms.append(used)
            optimizer.step()
            steps += 1
            st = detach(st)
            total = 0
        if not (stepped and faults.get("dones_before_detach")):
            st = mask(st, rows["dones"][t], faults)
    return dict(model=model, optimizer=optimizer, losses=losses, mean=sum(losses) / len(losses), grad_norm=norm, memory_grad_norm=mnorm, carry=detach(st),
                steps=steps, norms=norms)


def err(got, want):
    """e(t) = max|t - t64| / max|t64|."""
    want = torch.as_tensor(want).double()
    return float((torch.as_tensor(got).double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def bar(e32):
    return max(8.0 * e32, 2e-5)


def state_parts(state):
    """h, or (h, c) -> {"h": .., "c": ..}."""
    parts = _each(state)
    return {"h": parts[0], **({"c": parts[1]} if len(parts) > 1 else {})}


# ---- the cases of tests/test_hip_distill_recurrent_update.py
def group_cases(slab_rows, rnn):
    """Per memory type: nothing a multiple of 16; exact tiles with a single step; G * N a few rows past one weight-gradient slab; a non-zero carry
    with dones at the group's first, middle and last step (the group starts at time index 0, so it enters with the carry); hidden 344, where the
    backward tile takes two passes over the gate derivative's columns (K = 4 x 344 = 1376 for the LSTM, 3 x 344 = 1032 for the GRU)."""
    salt = 0 if rnn == "lstm" else 50
    return [
        Case(f"{rnn}_h40_n7_g3", rnn=rnn, salt=salt + 1),
        Case(f"{rnn}_h16_n16_g1", S=16, H=16, layers=1, mlp=(16,), A=16, N=16, G=1, rnn=rnn, loss="mse", salt=salt + 2),
        Case(f"{rnn}_h40_slab_g7", N=-(-(slab_rows + 3) // 7), G=7, rnn=rnn, salt=salt + 3),
        Case(f"{rnn}_h40_n7_g3_carry_dones", rnn=rnn, salt=salt + 4, dones_at={0: None, 1: None, 2: None}),
        Case(f"{rnn}_h344_n7_g3", H=344, rnn=rnn, salt=salt + 5),
    ]


CARRY_CASE = "carry_dones"          # the cases whose name ends so enter from carry_of(case)

# E = 2, T = 7, G = 3: groups (0 1 2) (3 4 5) (6 0 1) (2 3 4), remainder (5 6).  Dones at a group's first step (t = 3), at a group's last step
# (t = 2, 5 in epoch 0; t = 1, 4 in epoch 1) and at t = T - 1.
UPDATE_DONES = {1: (0, 3), 2: (1, 4), 3: (2, 5), 5: (0, 6), 6: (3, 4)}


def update_case(rnn, salt=20):
    return Case(f"{rnn}_update", N=7, G=3, T=7, rnn=rnn, salt=salt + (0 if rnn == "lstm" else 50), dones_at=UPDATE_DONES)


UPDATE_E, UPDATE_LR = 2, 2e-3
CLIP_SMALL, CLIP_LARGE = 0.05, 50.0          # every group's student.* norm lies between them (asserted in tests/test_distill_recurrent_update_reference.py)

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distillation_recurrent_update.npz")
GOLDEN_CASES = {          # tools/refgen/make_distillation_recurrent_update_golden.py -> tests/golden/distillation_recurrent_update.npz
    "lstm": dict(rnn="lstm", teacher_recurrent=False),
    "gru_teacher_recurrent": dict(rnn="gru", teacher_recurrent=True),
}
GOLDEN = dict(S=20, H=24, layers=2, mlp=(32, 16), A=12, N=7, T=7, G=3, E=2, lr=2e-3, loss="huber", rounds=2)


def seeded_moments(params, seed=8):
    """Non-zero Adam moments at step 7, for the optimiser-step checks."""
    g = torch.Generator().manual_seed(seed)
    return dict(exp_avg={k: 0.01 * torch.randn(v.shape, generator=g) for k, v in params.items()},
                exp_avg_sq={k: 1e-4 * torch.rand(v.shape, generator=g) for k, v in params.items()}, step=7)


def golden_state(z):
    """The fp32 state dict a golden case started from."""
    return {k[4:]: torch.from_numpy(z[k].astype(np.float32)) for k in z if k.startswith("sd0.")}


def golden_rows(z, r, tag="f32"):
    """The rows of round r as `collect_distillation` would return them; the targets are the teacher's of that precision's run."""
    return dict(observations=torch.from_numpy(z[f"r{r}.observations"]), teacher_observations=torch.from_numpy(z[f"r{r}.teacher_observations"]),
                privileged_actions=torch.from_numpy(z[f"r{r}.{tag}.privileged_actions"]), dones=torch.from_numpy(z[f"r{r}.dones"]))


def golden(name):
    """The reference's own record of a golden case: {key: array} with the `name.` prefix removed."""
    z = np.load(GOLDEN_FILE)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + ".")}
