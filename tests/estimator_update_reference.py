"""A torch-CPU restatement of the terrain estimator's update (`EstimatorDistillation.update`, `rsl_rl/algorithms/distillation.py:277-332`, as
include/lgestimator_train.h restates it) for the tests of `rl.NativeEstimatorDistillation`: group gradients and whole updates by autograd over
`tools/train_estimator.TerrainEstimatorTorch`, in float64 (the reference) and in float32 (torch's own rounding, which sets the bar).  No test here.

Inputs are closed-form or seeded: weights by `closed_form_state`, images by `closed_form_depth` -- the camera's [0, 1] range, or `6 (d - 0.5)` so that
the negative branches of ELU and tanh carry weight --, proprio rows and targets from a seeded generator.

The optional `faults` of `group_gradients` break the float64 reference in the ways the kernels can go wrong; tests/test_estimator_update_reference.py
shows that the bar of the GPU test sees each of them (its power)."""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.train_estimator import TerrainEstimatorTorch, closed_form_depth, closed_form_state          # noqa: E402

CONV_INDEX = (0, 2, 4, 6)          # depth_encoder[i]: the four convolutions
LOSSES = ("mse", "huber", "l1")


class Case:
    """One estimator and its rows.  shape: the image; N envs, T steps; G: the group length the tests use."""

    def __init__(self, name, shape, N, G, T=None, memory="gru", layers=1, act="elu", loss="mse", F=64, hidden=32, decoder=(24,), R=11, P=6, wide=True, salt=0,
                 dones_at=()):
        self.name, self.shape, self.N, self.G, self.T = name, tuple(shape), N, G, T or G
        self.memory, self.layers, self.act, self.loss, self.F, self.hidden, self.decoder, self.R, self.P = memory, layers, act, loss, F, hidden, tuple(decoder), R, P
        self.wide, self.salt, self.dones_at = wide, salt, tuple(dones_at)

    def module(self, dtype=torch.float32):
        m = TerrainEstimatorTorch(self.shape, self.P, self.R, encoder_output_dim=self.F, memory_hidden_size=self.hidden, memory_num_layers=self.layers,
                                  memory_type=self.memory, decoder_hidden_dims=self.decoder, activation=self.act)
        m.load_state_dict(closed_form_state(m, self.salt))
        return m.to(dtype)

    def state(self):
        return {k: v.clone() for k, v in self.module().state_dict().items()}

    def rows(self):
        """depth_images (T, N, h, w), proprio_data (T, N, P), raycast_targets (T, N, R), dones (T, N): fp32."""
        T, N = self.T, self.N
        d = closed_form_depth(T, N, *self.shape)
        if self.wide:
            d = (6.0 * (d.double() - 0.5)).float()
        g = torch.Generator().manual_seed(1234 + self.salt)
        prop = torch.randn(T, N, self.P, generator=g)
        # targets around what an untrained estimator predicts (|pred| < 1), spread so that |diff| lies on both sides of 1 (the Huber kink)
        tgt = 1.5 * torch.randn(T, N, self.R, generator=g)
        dones = torch.zeros(T, N)
        for t in self.dones_at:
            dones[t, (torch.arange(N) + t) % 2 == 0] = 1.0          # every other row, alternating with t (all rows of N = 1 at even t)
        return dict(depth_images=d, proprio_data=prop, raycast_targets=tgt, dones=dones)


def carry_of(case, seed=77):
    """A seeded non-zero state to enter with, so that weight_hh has a gradient in a group of one step: h, or (h, c)."""
    g = torch.Generator().manual_seed(seed + case.salt)
    h = 0.5 * torch.randn(case.layers, case.N, case.hidden, generator=g)
    return (h, 0.5 * torch.randn(case.layers, case.N, case.hidden, generator=g)) if case.memory == "lstm" else h


def loss_fn(name):
    return {"mse": F.mse_loss, "huber": F.huber_loss, "l1": F.l1_loss}[name]


def zero_state(case, dtype):
    h = torch.zeros(case.layers, case.N, case.hidden, dtype=dtype)
    return (h, h.clone()) if case.memory == "lstm" else h


def _each(state):
    return state if isinstance(state, tuple) else (state,)


def _like(state, parts):
    parts = tuple(parts)
    return parts if isinstance(state, tuple) else parts[0]


def detach(state):
    return _like(state, (s.detach() for s in _each(state)))


def cast(state, dtype):
    return _like(state, (s.detach().to(dtype).clone() for s in _each(state)))


def mask(state, dones):
    """`Memory.reset(dones)`: the rows with dones != 0 get zero state; no gradient crosses."""
    keep = (dones == 0).to(_each(state)[0].dtype).view(1, -1, 1)
    return _like(state, (s * keep for s in _each(state)))


# ---- faults: the convolution, the pooling and the activation with a backward pass that can be broken
class _FaultConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, faults, stage):
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, pad, faults, stage)
        return F.conv2d(x, w, b, stride, pad)

    @staticmethod
    def backward(ctx, d):
        x, w = ctx.saved_tensors
        stride, pad, faults, stage = ctx.cfg
        dd = d
        if faults.get("drop_last_pixel") == stage:           # the delta pixel at the map's last row / column is never read
            dd = d.clone(); dd[:, :, -1, :] = 0; dd[:, :, :, -1] = 0
        dw_d = dd
        if faults.get("slab_tail") == stage:                   # the last ragged rows (env, pixel) of the weight gradient's reduction are dropped
            flat = dd.permute(0, 2, 3, 1).reshape(-1, dd.shape[1]).clone()
            flat[-max(1, flat.shape[0] % 4 or 3):] = 0
            dw_d = flat.reshape(dd.shape[0], dd.shape[2], dd.shape[3], dd.shape[1]).permute(0, 3, 1, 2)
        wd = w
        if faults.get("tap_transposed") == stage:              # tap (0, 1) and tap (1, 0) exchanged in the transposed image
            wd = w.clone(); wd[:, :, 0, 1] = w[:, :, 1, 0]; wd[:, :, 1, 0] = w[:, :, 0, 1]
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.nn.grad.conv2d_input(x.shape, wd, dd, stride, pad)
            if faults.get("parity") == stage and stride == 2:  # the parity test of the stride-2 gather off by one: every input pixel gets its neighbour's sum
                dx = torch.roll(dx, shifts=(1, 1), dims=(2, 3))
        dw = torch.nn.grad.conv2d_weight(x, w.shape, dw_d, stride, pad)
        db = dw_d.sum(dim=(0, 2, 3))
        if faults.get("bias_high") == stage:                   # the bias gradient of channels >= 64
            db = db.clone(); db[64:] = 0
        return dx, dw, db, None, None, None, None


class _FaultPool(torch.autograd.Function):
    """AdaptiveAvgPool2d((4, 4)) whose backward floors the window END (the forward is torch's)."""

    @staticmethod
    def forward(ctx, x):
        ctx.shape = x.shape
        return F.adaptive_avg_pool2d(x, (4, 4))

    @staticmethod
    def backward(ctx, d):
        n, c, H, W = ctx.shape
        dx = torch.zeros(ctx.shape, dtype=d.dtype)
        for i in range(4):
            y0, y1 = (i * H) // 4, max(((i + 1) * H) // 4, (i * H) // 4 + 1)
            for j in range(4):
                x0, x1 = (j * W) // 4, max(((j + 1) * W) // 4, (j * W) // 4 + 1)
                dx[:, :, y0:y1, x0:x1] += d[:, :, i:i + 1, j:j + 1] / ((y1 - y0) * (x1 - x0))
        return dx


class _FaultAct(torch.autograd.Function):
    """The activation whose derivative takes the negative branch as 0."""

    @staticmethod
    def forward(ctx, x, name):
        y = {"elu": F.elu, "relu": F.relu, "tanh": torch.tanh}[name](x)
        ctx.save_for_backward(y)
        ctx.name = name
        return y

    @staticmethod
    def backward(ctx, d):
        y, = ctx.saved_tensors
        g = 1 - y * y if ctx.name == "tanh" else torch.ones_like(y)
        return d * torch.where(y > 0, g, torch.zeros_like(y)), None


def encode(model, case, depth, faults=None):
    """`model.depth_encoder` on (n, h, w) images; with faults, through the breakable pieces above."""
    if not faults:
        return model.encode(depth)
    enc, x = model.depth_encoder, depth.unsqueeze(1)
    shapes = ((2, 2), (2, 1), (2, 1), (1, 1))
    act = (lambda v: _FaultAct.apply(v, case.act)) if faults.get("act_negative") else enc[1]
    for stage, (i, (stride, pad)) in enumerate(zip(CONV_INDEX, shapes), start=1):
        x = act(_FaultConv.apply(x, enc[i].weight, enc[i].bias, stride, pad, faults, stage))
    x = _FaultPool.apply(x) if faults.get("pool_floor") else enc[8](x)
    x = enc[9](x)
    x = act(enc[10](x))
    return act(enc[12](x))


def step(model, case, rows, t, state, faults=None):
    """One step of every row at time index t from `state`: (predictions, new state)."""
    x = model.combination_mlp(torch.cat([encode(model, case, rows["depth_images"][t], faults), rows["proprio_data"][t]], dim=-1))
    out, state = model.memory.rnn(x.unsqueeze(0), state)
    return model.decoder(out.squeeze(0)), state


def to_dtype(rows, dtype):
    return {k: v.to(dtype) for k, v in rows.items()}


def global_norm(model):
    return torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters())).item()


def named_grads(model):
    """The gradients in the state dict's names."""
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def group_gradients(case, dtype=torch.float64, first_step=0, num_steps=None, enter=None, carry=None, use_dones=False, faults=None, state=None, pre_steps=0):
    """The gradient of the SUM of the losses of steps [first_step, first_step + num_steps): (grads by name, global norm, step losses, predictions
    (steps, N, R), the state after the last step).  enter: the state the first step enters with when its time index is not 0 (zeros if None);
    carry: the state a step with time index 0 enters with (zeros if None).  faults: see the module docstring; "bptt_cut": the chain is cut
    between the steps of the group.  pre_steps: that many steps before first_step are run first, with the same weights and without a loss, to
    produce the entering state -- as a constant, unless the fault "no_detach" leaves the chain uncut at the group's first step."""
    faults = faults or {}
    model = case.module(dtype)
    if state is not None:
        model.load_state_dict({k: v.to(dtype) for k, v in state.items()})
    rows, fn = to_dtype(case.rows(), dtype), loss_fn(case.loss)
    nsteps = case.G if num_steps is None else num_steps
    st = cast(enter, dtype) if enter is not None else zero_state(case, dtype)
    for s in range(-pre_steps, 0):
        t = (first_step + s) % case.T
        if t == 0:
            st = cast(carry, dtype) if carry is not None else zero_state(case, dtype)
        st = step(model, case, rows, t, st)[1]
        if use_dones:
            st = mask(st, rows["dones"][t])
    if pre_steps and not faults.get("no_detach"):
        st = detach(st)
    total, losses, preds = 0, [], []
    for s in range(nsteps):
        t = (first_step + s) % case.T
        if t == 0:
            st = cast(carry, dtype) if carry is not None else zero_state(case, dtype)
        elif faults.get("bptt_cut") and s > 0:
            st = detach(st)
        pred, st = step(model, case, rows, t, st, faults)
        l = fn(pred, rows["raycast_targets"][t])
        total = total + l
        losses.append(l.item()); preds.append(pred.detach())
        if use_dones:
            st = mask(st, rows["dones"][t])
    model.zero_grad()
    total.backward()
    return named_grads(model), global_norm(model), losses, torch.stack(preds), detach(st)


def run_update(case, dtype=torch.float64, E=1, G=None, lr=1e-3, max_grad_norm=None, use_dones=False, carry=None, model=None, optimizer=None, faults=None, rows=None):
    """A whole update.  Returns dict: model, optimizer, losses (E T), mean, grad_norm (of the last optimiser step, None if none), carry, steps.
    rows: other rows than the case's own (same shapes).  faults: "epoch_chain": an epoch starts from the previous epoch's end."""
    faults = faults or {}
    G = G or case.G
    if model is None:
        model = case.module(dtype)
        optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    rows, fn = to_dtype(rows if rows is not None else case.rows(), dtype), loss_fn(case.loss)
    T = case.T
    carry0 = cast(carry, dtype) if carry is not None else zero_state(case, dtype)
    st, total, losses, cnt, norm, steps = carry0, 0, [], 0, None, 0
    for k in range(E * T):
        t = k % T
        if t == 0 and not (faults.get("epoch_chain") and k > 0):
            st = carry0
        pred, st = step(model, case, rows, t, st)
        l = fn(pred, rows["raycast_targets"][t])
        total = total + l
        losses.append(l.item())
        cnt += 1
        if cnt % G == 0:
            optimizer.zero_grad()
            total.backward()
            norm = global_norm(model)
            if max_grad_norm:
                nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)
            optimizer.step()
            steps += 1
            st = detach(st)
            total = 0
        if use_dones:
            st = mask(st, rows["dones"][t])
    return dict(model=model, optimizer=optimizer, losses=losses, mean=sum(losses) / len(losses), grad_norm=norm, carry=detach(st), steps=steps)


def predict(model, case, rows, t=0):
    """The module's predictions on the rows of time index t from zero state (a probe of the trained weights)."""
    dtype = next(model.parameters()).dtype
    with torch.no_grad():
        return step(model, case, to_dtype(rows, dtype), t, zero_state(case, dtype))[0]


def err(got, want):
    """e(t) = max|t - t64| / max|t64|."""
    want = want.double()
    return float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def bar(e32):
    return max(8.0 * e32, 2e-5)


# ---- the cases of tests/test_hip_estimator_update.py's group test (the slab case is built there, from the library's slab size)
def group_cases():
    return [
        Case("8x8_n1_g1", (8, 8), 1, 1),
        Case("9x11_n2_g2_lstm", (9, 11), 2, 2, memory="lstm", loss="huber", salt=1),
        Case("8x128_n3_g1", (8, 128), 3, 1, act="relu", salt=2),
        Case("128x8_n3_g1", (128, 8), 3, 1, act="tanh", loss="l1", salt=3),
        Case("29x57_n3_g2", (29, 57), 3, 2, F=40, salt=4),
        Case("29x57_n70_g3_gru2", (29, 57), 70, 3, layers=2, salt=5),
        Case("58x87_n33_g2", (58, 87), 33, 2, loss="huber", salt=6),
        Case("28x56_n70_g15_registered", (28, 56), 70, 15, hidden=256, decoder=(128, 64), R=81, salt=7),
        Case("9x11_n3_g3_dones", (9, 11), 3, 3, T=4, dones_at=(0, 1, 2, 3), salt=8),
    ]


def slab_case(slab_rows):
    """9 x 11 images: 30, 9, 4 and 4 output pixels per env.  N = 2 slabs / 4 + 3 envs: conv 3 and conv 4 have two full slabs and a ragged third of 12
    rows, conv 1 and conv 2 more full slabs and a ragged last one, and 9 pixels per env put env boundaries inside conv 2's slabs."""
    return Case("9x11_slabs", (9, 11), 2 * slab_rows // 4 + 3, 1, hidden=16, decoder=(), R=5, salt=9)


OPT_CASE = dict(name="29x57_opt", shape=(29, 57), N=3, G=2, salt=4)
CLIP_SMALL, CLIP_LARGE = 0.5, 50.0          # the group's norm lies between them (asserted in tests/test_estimator_update_reference.py)
UPDATE_CASE = dict(name="9x11_update", shape=(9, 11), N=3, G=3, T=4, salt=10)          # E = 2: groups (0 1 2) (3 0 1), remainder (2 3)


GOLDEN_CASES = {          # tools/refgen/make_estimator_update_golden.py -> tests/golden/estimator_update.npz
    "gru_mse_clip": dict(case=dict(memory="gru", loss="mse", **UPDATE_CASE), E=1, lr=2e-3, max_grad_norm=1.0),
    "lstm_huber": dict(case=dict(memory="lstm", loss="huber", **UPDATE_CASE), E=2, lr=2e-3, max_grad_norm=None),
}


def golden(name):
    """The reference's own figures of a golden case: {"f32" | "f64": {loss, step_losses, grad_norm, probe, norms}}."""
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "estimator_update.npz"))
    return {tag: {k: z[f"{name}.{tag}.{k}"] for k in ("loss", "step_losses", "grad_norm", "probe", "norms")} for tag in ("f32", "f64")}
