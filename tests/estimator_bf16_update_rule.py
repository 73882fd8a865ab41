"""The rule the bf16 trainer of the terrain estimator follows (include/lgestimator_train_bf16.h), restated in torch on the CPU for the tests of
`NativeEstimatorDistillation(encoder_training="bf16")`.  It builds on tests/estimator_update_reference.py (cases, rows, losses, the memory's handling,
the faults) and on `R` of tests/bf16_encoder_rule.py.  No test here.

R(v): v rounded to bf16, nearest even.  The function that is differentiated: the module with R on the image, on the encoder's six weight tensors and on
the outputs of stages 1-6 (conv 1-4, pool + flatten, linear 1); biases, bias add, activation, accumulation and everything behind the encoder in the
working dtype.  Rounding is straight-through; an activation's derivative is taken from its stored (rounded) output with the kernels' formulas.

    rule reference   float64, no delta rounding: `group_gradients(case, torch.float64)`
    fp32 emulation   the same in float32, and the deltas with a map's shape (w.r.t. the pre-activations of conv 1-4) through R, each once:
                     `group_gradients(case, torch.float32, round_deltas=True)`
    stages           the float64 backward of ONE stage on given operands (`stage_backward`), optionally with a fault of the reference"""
import torch
import torch.nn.functional as F

from tests import estimator_update_reference as ref
from tests.bf16_encoder_rule import R

CONV_SHAPES = ((2, 2), (2, 1), (2, 1), (1, 1))          # (stride, padding) of conv 1-4


def act_grad(y, name):
    """est_act_grad: the derivative of the activation from its OUTPUT."""
    if name == "relu":
        return (y > 0).to(y.dtype)
    if name == "tanh":
        return 1 - y * y
    return torch.where(y > 0, torch.ones_like(y), y + 1)          # ELU


def act_fn(name):
    return {"elu": F.elu, "relu": F.relu, "tanh": torch.tanh}[name]


class _RoundST(torch.autograd.Function):
    """R, straight-through."""

    @staticmethod
    def forward(ctx, x):
        return R(x)

    @staticmethod
    def backward(ctx, d):
        return d


class _ActStored(torch.autograd.Function):
    """y = act(z), stored through R if `rounded`; backward d * act'(stored y), through R if `round_delta`."""

    @staticmethod
    def forward(ctx, z, name, rounded, round_delta):
        y = act_fn(name)(z)
        if rounded:
            y = R(y)
        ctx.save_for_backward(y)
        ctx.cfg = (name, round_delta)
        return y

    @staticmethod
    def backward(ctx, d):
        y, = ctx.saved_tensors
        name, round_delta = ctx.cfg
        g = d * act_grad(y, name)
        return (R(g) if round_delta else g), None, None, None


def encode(model, case, depth, round_deltas=False):
    """The bf16 encoder's function on (n, h, w) images, in the module's dtype."""
    enc = model.depth_encoder
    x = R(depth).unsqueeze(1)
    for i, (stride, pad) in zip(ref.CONV_INDEX, CONV_SHAPES):
        x = _ActStored.apply(F.conv2d(x, _RoundST.apply(enc[i].weight), enc[i].bias, stride, pad), case.act, True, round_deltas)
    x = _RoundST.apply(F.adaptive_avg_pool2d(x, (4, 4)).flatten(1))
    x = _ActStored.apply(F.linear(x, _RoundST.apply(enc[10].weight), enc[10].bias), case.act, True, False)
    return _ActStored.apply(F.linear(x, _RoundST.apply(enc[12].weight), enc[12].bias), case.act, False, False)


def step(model, case, rows, t, state, round_deltas=False):
    x = model.combination_mlp(torch.cat([encode(model, case, rows["depth_images"][t], round_deltas), rows["proprio_data"][t]], dim=-1))
    out, state = model.memory.rnn(x.unsqueeze(0), state)
    return model.decoder(out.squeeze(0)), state


def group_gradients(case, dtype=torch.float64, round_deltas=False, first_step=0, num_steps=None, enter=None, carry=None, use_dones=False, state=None):
    """`estimator_update_reference.group_gradients` for the rule: (grads by name, global norm, step losses, predictions, the state after the last step)."""
    model = case.module(dtype)
    if state is not None:
        model.load_state_dict({k: v.to(dtype) for k, v in state.items()})
    rows, fn = ref.to_dtype(case.rows(), dtype), ref.loss_fn(case.loss)
    nsteps = case.G if num_steps is None else num_steps
    st = ref.cast(enter, dtype) if enter is not None else ref.zero_state(case, dtype)
    total, losses, preds = 0, [], []
    for s in range(nsteps):
        t = (first_step + s) % case.T
        if t == 0:
            st = ref.cast(carry, dtype) if carry is not None else ref.zero_state(case, dtype)
        pred, st = step(model, case, rows, t, st, round_deltas)
        l = fn(pred, rows["raycast_targets"][t])
        total = total + l
        losses.append(l.item()); preds.append(pred.detach())
        if use_dones:
            st = ref.mask(st, rows["dones"][t])
    model.zero_grad()
    total.backward()
    return ref.named_grads(model), ref.global_norm(model), losses, torch.stack(preds), ref.detach(st)


# ---- one backward stage in float64 on given operands
def stage_backward(kind, act, delta, x=None, w=None, y_below=None, stride=1, pad=0, faults=None, stage=0):
    """The float64 backward of one stage.  Operands as torch holds them: maps (n, C, H, W), rows (n, width).
    kind "pool":   delta (n, 1024) w.r.t. the pooled rows, y_below = conv 4's stored output -> d w.r.t. conv 4's pre-activation
    kind "conv":   delta (n, C_out, H', W') w.r.t. the pre-activation, x the layer's stored input, w its weights (after R), y_below = x as the
                   stored output of the layer below (None: the image, no data gradient) -> (dX w.r.t. the pre-activation below | None, dW, db)
    kind "linear": delta (n, dO), x (n, dI), w (dO, dI), y_below (None: no activation below) -> (dX, dW, db)
    faults / stage: a fault of tests/estimator_update_reference.py, applied when it names `stage`."""
    faults = faults or {}
    delta = delta.double()
    if kind == "pool":
        y = y_below.double().requires_grad_(True)
        pooled = (ref._FaultPool.apply(y) if faults.get("pool_floor") else F.adaptive_avg_pool2d(y, (4, 4))).flatten(1)
        d, = torch.autograd.grad(pooled, y, delta)
        return (d * _stored_grad(y_below.double(), act, faults)).detach()
    if kind == "conv":
        xx = x.double().requires_grad_(y_below is not None)
        ww = w.double().requires_grad_(True)
        bb = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
        out = ref._FaultConv.apply(xx, ww, bb, stride, pad, faults, stage)
        if y_below is not None:
            dx, dw, db = torch.autograd.grad(out, (xx, ww, bb), delta)
            return dx * _stored_grad(y_below.double(), act, faults), dw, db
        dw, db = torch.autograd.grad(out, (ww, bb), delta)
        return None, dw, db
    dx = delta @ w.double()
    if y_below is not None:
        dx = dx * _stored_grad(y_below.double(), act, faults)
    return dx, delta.t() @ x.double(), delta.sum(0)


def _stored_grad(y, act, faults):
    g = act_grad(y, act)
    return torch.where(y > 0, g, torch.zeros_like(g)) if faults.get("act_negative") else g


def stage_backward32(kind, act, delta, x=None, w=None, y_below=None, stride=1, pad=0):
    """torch fp32 on the same operands: the gap of the interval rule, e32 of the fp32 bar."""
    delta = delta.float()
    if kind == "pool":
        y = y_below.float().requires_grad_(True)
        d, = torch.autograd.grad(F.adaptive_avg_pool2d(y, (4, 4)).flatten(1), y, delta)
        return (d * act_grad(y_below.float(), act)).detach()
    if kind == "conv":
        dw = torch.nn.grad.conv2d_weight(x.float(), w.shape, delta, stride, pad)
        db = delta.sum(dim=(0, 2, 3))
        if y_below is None:
            return None, dw, db
        return torch.nn.grad.conv2d_input(x.shape, w.float(), delta, stride, pad) * act_grad(y_below.float(), act), dw, db
    dx = delta @ w.float()
    if y_below is not None:
        dx = dx * act_grad(y_below.float(), act)
    return dx, delta.t() @ x.float(), delta.sum(0)
