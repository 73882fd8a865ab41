"""What tests/test_rnn_sweep_power.py (CPU) and tests/test_hip_rnn_sweep.py (GPU) share: the memory shapes, weights, inputs, the float64 reference and
the bar of the sweep of `lg_rnn_step`, `lg_rnn_reset_rows` and `lg_policy_act_recurrent` (csrc/lg_rnn_tile.h: `rnn_tile`, `rnn_blocks`).  No GPU, no
test functions.

Reference: `step`, one step of an `nn.LSTM` / `nn.GRU` stack in plain numpy (float64; the same code in float32 is the yardstick) with
`Memory.reset(dones)` folded in: a row whose reset flag is set enters with h = 0 and c = 0 on every layer.  Gate order i f g o / r z n; a GRU's b_hn
sits inside r * (W_hn h + b_hn).  The hooks break it in the ways the tile can go wrong (tests/test_rnn_sweep_power.py).
Weights: uniform, bound 1.7 / sqrt(fan_in) -- fan_in is the input width for weight_ih of layer 0 and the hidden width for every other matrix -- and
biases uniform in +-0.5: pre-activations O(1) at every width (torch's 1 / sqrt(H) for weight_ih saturates the gates at 512 inputs, 24 units).
Inputs: STEPS = 3 steps of seeded randn rows; the rows of a smaller n are the first rows of the largest.  At step 1 about 30 % of the rows are reset,
among them row 0, row 31 and the last row of every n in ROWS.  The state starts from zero.
Bar: the project's rule for this path (tests/test_hip_policy_recurrent.py), max(2e-5, 4 x yardstick), absolute, on every layer's h' and c' after every
step; `case` asserts that the floor binds and that the states are O(1), so a later change of the inputs cannot loosen the bar unnoticed."""
import functools

import numpy as np
import torch

FLOOR, POWER = 2e-5, 10.0
ROWS = (1, 31, 32, 33, 70)              # 70: two full 32-row tiles and a ragged third
MAX_ROWS = max(ROWS)
STEPS, RESET_STEP = 3, 1
TYPES = ("lstm", "gru")
KMAX, CHUNK_WAVES, MAX_LAYERS = 1024, 8, 4          # RNN_KMAX, MLP_THREADS / 64, RNN_MAX_LAYERS
SHAPES = [(1, 1, 1), (17, 15, 1), (15, 17, 3), (16, 16, 4), (33, 9, 2), (64, 129, 1), (48, 144, 2), (235, 257, 1), (512, 24, 1), (1, 512, 1),          # (inputs I, hidden H, layers L)
          (511, 511, 1), (512, 512, 1)]
CASES = [(rnn, shape) for shape in SHAPES for rnn in TYPES]
# (actor memory, critic memory) through lg_policy_act_recurrent: equal depth and different widths (side by side on blockIdx.y); different depths (one after the other)
PAIRS = [((15, 17, 3), (33, 9, 3)), ((64, 129, 1), (48, 144, 2))]
PAIR_ROWS, PAIR_ACTIONS, HEAD_WIDTH = 33, 5, 16
TRAIN_SHAPES = [(15, 17, 3), (64, 129, 1), (235, 257, 1), (511, 511, 1)]          # the training forward against the act, T = 3, 33 envs
TRAIN_T, TRAIN_ENVS = 3, 33

# Weight sets the power test (tests/test_rnn_sweep_power.py) turned down, with what was under ten bars there at salt 0; the next salt passes
SALTS = {}


def gates(rnn):
    return 4 if rnn == "lstm" else 3


def case_id(rnn, shape):
    return rnn + "-" + "-".join(str(d) for d in shape)


def tiling(shape):
    """What `rnn_create` derives from a shape, per layer: dict(nbx, nbh, Kp, nch)."""
    I, H, L = shape
    out = []
    for l in range(L):
        Ip, Hp = ((I if l == 0 else H) + 15) // 16 * 16, (H + 15) // 16 * 16
        out.append(dict(nbx=Ip // 16, nbh=Hp // 16, Kp=Ip + Hp, nch=Hp // 16))
    return out


def _seed(rnn, shape, salt):
    return (sum((i + 1) * 7919 * d for i, d in enumerate(shape)) + 15485863 * gates(rnn) + 104729 * salt) % (2 ** 31)


def make_layers(rnn, shape, salt=0):
    """Per layer (weight_ih (G H, I), weight_hh (G H, H), bias_ih (G H), bias_hh (G H)) in torch's layout, fp32 numpy."""
    I, H, L = shape
    G, g, out = gates(rnn), torch.Generator().manual_seed(_seed(rnn, shape, salt)), []

    def uniform(bound, *size):
        return ((torch.rand(*size, generator=g) * 2 - 1) * bound).numpy().astype(np.float32)
    for l in range(L):
        K = I if l == 0 else H
        out.append((uniform(1.7 / np.sqrt(I if l == 0 else H), G * H, K), uniform(1.7 / np.sqrt(H), G * H, H), uniform(0.5, G * H), uniform(0.5, G * H)))
    return out


def make_rows(width, n=MAX_ROWS, salt=0):
    """(STEPS, n, width) fp32 randn rows: the first n of the MAX_ROWS rows this (width, salt) always gives."""
    g = torch.Generator().manual_seed(_seed("lstm", (width,), 1000 + salt))
    return torch.randn(STEPS, MAX_ROWS, width, generator=g)[:, :n].contiguous()


def reset_mask(n=MAX_ROWS):
    """(n) fp32, 1 where the row is reset at RESET_STEP: the first n entries of one fixed mask of MAX_ROWS rows that holds row 0, row 31 and the last row
    of every n in ROWS, about 30 % in all."""
    g = torch.Generator().manual_seed(977)
    m = (torch.rand(MAX_ROWS, generator=g) < 0.25).float()
    for r in {0, 31} | {k - 1 for k in ROWS}:
        m[r] = 1.0
    return m[:n].contiguous()


# ------------------------------------------------------------------------------------------------ the reference
def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def step(rnn, layers, x, h, c, reset=None, dtype=np.float64, hooks=None):
    """One step of the stack.  x (n, I); h, c (L, n, H) (c None for a GRU); reset (n) or None.  Returns (h', c') in `dtype`.

    hooks (all optional; l is the layer):
      pre_x[l](x)        edits the input the layer's weight_ih product reads
      pre_h[l](h)        edits the entering state the layer's weight_hh product reads
      swap_gates         the first two gates exchanged (i <-> f, r <-> z)
      bhn_outside        a GRU's b_hn added outside r * (...)
      carry_unmasked     a GRU's z * h takes the h of before the reset mask
      keep_c             c is not zeroed on a reset row
      stale_below        layer l >= 1 reads the h of layer l - 1 from before this step
      post(h', c')       edits the new state of the whole stack"""
    hooks = hooks or {}
    H = h.shape[2]
    x, h = np.asarray(x, dtype), np.asarray(h, dtype)
    c = np.asarray(c, dtype) if rnn == "lstm" else None
    keep = np.ones((x.shape[0], 1), dtype) if reset is None else (np.asarray(reset) == 0).astype(dtype)[:, None]
    hn, cn, inp = [], [], x
    for l, (wi, wh, bi, bh) in enumerate(layers):
        wi, wh, bi, bh = (np.asarray(a, dtype) for a in (wi, wh, bi, bh))
        if l > 0 and hooks.get("stale_below"):
            inp = h[l - 1]
        hin = h[l] * keep
        xa = hooks["pre_x"][l](inp.copy()) if l in hooks.get("pre_x", {}) else inp
        ha = hooks["pre_h"][l](hin.copy()) if l in hooks.get("pre_h", {}) else hin
        gi, gh = xa @ wi.T + bi, ha @ wh.T + bh
        a, b = (1, 0) if hooks.get("swap_gates") else (0, 1)
        if rnn == "lstm":
            g = gi + gh
            i, f, gg, o = sigmoid(g[:, a * H:(a + 1) * H]), sigmoid(g[:, b * H:(b + 1) * H]), np.tanh(g[:, 2 * H:3 * H]), sigmoid(g[:, 3 * H:])
            cin = c[l] if hooks.get("keep_c") else c[l] * keep
            c2 = f * cin + i * gg
            h2 = o * np.tanh(c2)
            cn.append(c2)
        else:
            r, z = sigmoid(gi[:, a * H:(a + 1) * H] + gh[:, a * H:(a + 1) * H]), sigmoid(gi[:, b * H:(b + 1) * H] + gh[:, b * H:(b + 1) * H])
            if hooks.get("bhn_outside"):
                n = np.tanh(gi[:, 2 * H:] + r * (gh[:, 2 * H:] - bh[2 * H:]) + bh[2 * H:])
            else:
                n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            h2 = (1 - z) * n + z * (h[l] if hooks.get("carry_unmasked") else hin)
        hn.append(h2)
        inp = h2
    hn, cn = np.stack(hn).astype(dtype), (np.stack(cn).astype(dtype) if rnn == "lstm" else None)
    if "post" in hooks:
        hn, cn = hooks["post"](hn, cn)
    return hn, cn


def run(rnn, layers, x, reset, dtype=np.float64, hooks=None):
    """STEPS steps from a zero state, the reset at RESET_STEP: [(h', c') after each step], h' (L, n, H)."""
    x = np.asarray(x)
    L, H, n = len(layers), layers[0][1].shape[1], x.shape[1]
    h, c, out = np.zeros((L, n, H), dtype), (np.zeros((L, n, H), dtype) if rnn == "lstm" else None), []
    for t in range(x.shape[0]):
        h, c = step(rnn, layers, x[t], h, c, reset if t == RESET_STEP else None, dtype, hooks)
        out.append((h, c))
    return out


def states(trace):
    """Every tensor of a `run`: [(step, 'h' | 'c', (L, n, H) array)]."""
    return [(t, tag, a) for t, hc in enumerate(trace) for tag, a in zip("hc", hc) if a is not None]


def deviation(trace, want):
    return max(float(np.abs(np.asarray(a, np.float64) - b).max()) for (_, _, a), (_, _, b) in zip(states(trace), states(want)))


def bar_of(yardstick):
    return max(FLOOR, 4.0 * yardstick)


@functools.lru_cache(maxsize=None)
def _case(rnn, shape, salt):
    layers, x, reset = make_layers(rnn, shape, salt), make_rows(shape[0], salt=salt), reset_mask()
    want = run(rnn, layers, x.numpy(), reset.numpy())
    yardstick = deviation(run(rnn, layers, x.numpy(), reset.numpy(), np.float32), want)
    top = max(float(np.abs(a).max()) for _, _, a in states(want))
    assert 4.0 * yardstick <= FLOOR, f"{case_id(rnn, shape)}: the fp32 restatement is {yardstick:.3e} from float64: the 2e-5 floor no longer binds"
    assert 0.05 <= top <= 20.0, f"{case_id(rnn, shape)}: states are not O(1): max {top:.3e}"
    for _, _, a in states(want):
        a.setflags(write=False)
    return layers, x, reset, want, yardstick, bar_of(yardstick)


def case(rnn, shape, salt=None):
    """(layers, rows (STEPS, MAX_ROWS, I) fp32 torch, reset (MAX_ROWS) fp32 torch, float64 states per step (read-only), yardstick, bar); computed once."""
    shape = tuple(shape)
    return _case(rnn, shape, SALTS.get(case_id(rnn, shape), 0) if salt is None else salt)


# ------------------------------------------------------------------------------------------------ policies around the memories
def make_head(H, out, salt):
    """An MLP [H, HEAD_WIDTH, out] as [(weight, bias)], fp32 numpy: the weight rule of tests/policy_sweep.py."""
    g, dims, layers = torch.Generator().manual_seed(_seed("gru", (H, out), 2000 + salt)), [H, HEAD_WIDTH, out], []
    for j in range(2):
        bound = 1.0 / np.sqrt(dims[j])
        layers.append((((torch.rand(dims[j + 1], dims[j], generator=g) * 2 - 1) * bound * 1.7).numpy(), ((torch.rand(dims[j + 1], generator=g) * 2 - 1) * bound).numpy()))
    return layers


def policy_state(rnn, actor_shape, critic_shape, salt=0):
    """An `ActorCriticRecurrent` state dict: the sweep's memories of the two shapes (critic at salt + 1) in front of heads [H, 16, A] / [H, 16, 1]."""
    sd = {}
    for prefix, head, shape, out, s in (("memory_a", "actor", actor_shape, PAIR_ACTIONS, salt), ("memory_c", "critic", critic_shape, 1, salt + 1)):
        for l, layer in enumerate(make_layers(rnn, shape, s)):
            for name, a in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), layer):
                sd[f"{prefix}.rnn.{name}_l{l}"] = torch.from_numpy(a)
        for j, (w, b) in enumerate(make_head(shape[1], out, s)):
            sd[f"{head}.{2 * j}.weight"], sd[f"{head}.{2 * j}.bias"] = torch.from_numpy(w), torch.from_numpy(b)
    sd["std"] = torch.linspace(0.3, 1.1, PAIR_ACTIONS)
    return sd


def memory_layers(sd, prefix):
    L = len([k for k in sd if k.startswith(prefix + ".rnn.weight_ih_l")])
    return [tuple(sd[f"{prefix}.rnn.{name}_l{l}"].numpy() for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(L)]


def head_layers(sd, prefix):
    return [(sd[f"{prefix}.{2 * j}.weight"].numpy(), sd[f"{prefix}.{2 * j}.bias"].numpy()) for j in range(2)]


def pair_dones(n=PAIR_ROWS):
    """(STEPS, n) fp32: the dones `reset` takes after each step; about a third of the rows, the first and the last among them at some step."""
    g = torch.Generator().manual_seed(733)
    d = (torch.rand(STEPS, n, generator=g) < 0.3).float()
    d[0, 0] = d[1, n - 1] = d[0, min(31, n - 1)] = 1.0
    return d
