"""What tests/test_policy_sweep_power.py (CPU) and tests/test_hip_policy_sweep.py (GPU) share: the network shapes, weights, inputs, the float64 reference
and the bar of the sweep of `lg_mlp_forward`, `lg_policy_act`, `lg_distill_act` and `lg_compute_returns`.  No GPU, no test functions.

Weights: the rule of tests/test_hip_ppo_update.py::_random_sd -- uniform, bound 1.7 / sqrt(fan_in), bias bound 1 / sqrt(fan_in) -- which keeps the
activations O(1) through any depth.  Inputs: randn rows from a fixed seed; the rows of a smaller n are the first rows of the largest.
Reference: oracle.policy_oracle.mlp_forward (numpy float64).  Yardstick: the same network in torch fp32 on the CPU against it.
Bar: the project's rule, max(2e-5, 4 x yardstick), absolute; the yardstick is 1e-07 to 1.7e-06 on these shapes, so the floor binds everywhere, and
`case` asserts that it does: a later change of the inputs cannot loosen the bar unnoticed."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import policy_oracle as po

FLOOR, POWER = 2e-5, 10.0
DRAW_BAR = 2e-5                         # on z: the bar tests/test_traj_sampler.py holds the planner's draw to
ROWS = (1, 31, 32, 33, 70)              # 70: two full 32-row tiles and a ragged third
MAX_ROWS = max(ROWS)
ACTS = ("elu", "relu", "tanh", "lrelu", "selu")
DEEP = [20] + [24] * 7 + [6]            # L = 8 = LG_MLP_MAX_LAYERS
DIMS = [[1, 1], [63, 17], [64, 16], [65, 33], [8, 100], [8, 512],                                    # L = 1: no hidden layer, no buffer swap
        [16, 64, 12], [17, 65, 1], [5, 192, 7], [48, 1, 1, 3], [128, 512, 1], [512, 512, 32],
        [45, 70, 33, 7], [235, 129, 63, 12], DEEP]
EVERY_ACT_DIMS = [[17, 65, 1], [5, 192, 7], [45, 70, 33, 7], DEEP]
FORWARD_CASES = [(d, "elu") for d in DIMS] + [(d, a) for a in ACTS[1:] for d in EVERY_ACT_DIMS]

# (actor dims, critic dims): different depths and observation widths; the teacher of lg_distill_act is the critic's body ending in the action count
ACT_PAIRS = [([17, 65, 1], [51, 20, 10, 1]), ([5, 2], [9, 33, 17, 1]), ([45, 70, 33, 7], [51, 20, 1]), ([64, 16], [48, 64, 32, 1]),
             ([63, 100, 17], [8, 1]), ([235, 129, 63, 31], [128, 512, 1]), ([512, 512, 32], [20, 24, 24, 1])]
ACT_ROWS = (1, 33, 70)
DRAW_SEED = 0x1234_5678_9ABC            # both key words in use
DRAW_CALLS = (1, 7, (1 << 32) + 7)      # the last one: call_hi != 0, and its low word equals call 7

_TORCH_ACT = {"elu": F.elu, "relu": F.relu, "tanh": torch.tanh, "lrelu": lambda x: F.leaky_relu(x, 0.01), "selu": F.selu}


def case_id(dims, act):
    return "-".join(str(d) for d in dims) + "-" + act


def teacher_dims(critic_dims, num_actions):
    return list(critic_dims[:-1]) + [num_actions]


def _seed(dims, salt):
    return (sum((i + 1) * 7919 * d for i, d in enumerate(dims)) + 104729 * salt) % (2 ** 31)


def make_layers(dims, salt=0):
    """[(weight (out, in), bias (out))] as fp32 numpy arrays."""
    g = torch.Generator().manual_seed(_seed(dims, salt))
    out = []
    for j in range(len(dims) - 1):
        bound = 1.0 / np.sqrt(dims[j])
        w = (torch.rand(dims[j + 1], dims[j], generator=g) * 2 - 1) * bound * 1.7
        b = (torch.rand(dims[j + 1], generator=g) * 2 - 1) * bound
        out.append((w.numpy().astype(np.float32), b.numpy().astype(np.float32)))
    return out


def make_rows(width, n=MAX_ROWS, salt=0):
    """(n, width) fp32 randn rows: the first n of the MAX_ROWS rows this (width, salt) always gives."""
    g = torch.Generator().manual_seed(_seed([width], 1000 + salt))
    return torch.randn(MAX_ROWS, width, generator=g)[:n].contiguous()


def std_vector(num_actions):
    """A non-uniform `std` parameter."""
    return torch.linspace(0.3, 1.1, num_actions) if num_actions > 1 else torch.tensor([0.7])


def torch_forward(layers, x, act, dtype=torch.float32):
    h = x.to(dtype)
    for i, (w, b) in enumerate(layers):
        h = F.linear(h, torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype))
        if i < len(layers) - 1:
            h = _TORCH_ACT[act](h)
    return h


def bar_of(yardstick):
    return max(FLOOR, 4.0 * yardstick)


@functools.lru_cache(maxsize=None)
def _case(dims, act, salt):
    layers, x = make_layers(list(dims), salt), make_rows(dims[0], salt=salt)
    want = po.mlp_forward(layers, x.numpy(), act)
    yardstick = float(np.abs(torch_forward(layers, x, act).double().numpy() - want).max())
    assert 4.0 * yardstick <= FLOOR, f"{case_id(dims, act)}: torch fp32 is {yardstick:.3e} from float64: the 2e-5 floor no longer binds"
    assert 0.05 <= float(np.abs(want).max()) <= 20.0, f"{case_id(dims, act)}: outputs are not O(1): max {float(np.abs(want).max()):.3e}"
    want.setflags(write=False)
    return layers, x, want, yardstick, bar_of(yardstick)


# Weight sets the power test (tests/test_policy_sweep_power.py) turned down, with what was under ten bars there at salt 0; the next salt passes
SALTS = {"48-1-1-3-elu": 1,                            # the activation left out after layer 1: 0.0 bars
         "128-512-1-elu": 1,                           # the bias of column 511 of layer 0: 0.1 bars
         "20-24-24-24-24-24-24-24-6-lrelu": 1}         # three biases at 3 to 5 bars (units that are negative, so scaled by 0.01, on every row)


def case(dims, act="elu", salt=None):
    """(layers, rows (MAX_ROWS, dims[0]) fp32 torch, float64 outputs (read-only), yardstick, bar) of one network of the sweep; computed once."""
    return _case(tuple(dims), act, SALTS.get(case_id(dims, act), 0) if salt is None else salt)


# ------------------------------------------------------------------------------------------------ pointwise activations
def activation_grid():
    """Normal fp32 numbers: 0, +-1e-6 ... +-30 log-spaced, a dense linear stretch over [-0.3, 0.05], and the neighbours of ELU's two switch points."""
    mags = np.logspace(-6, np.log10(30.0), 600).astype(np.float32)
    tiny = np.finfo(np.float32).tiny                   # the neighbours of 0 among the normal numbers: +-2**-126 (nextafter(0) itself is denormal)
    near = [np.float32(-0.25), tiny, -tiny]
    lo = hi = np.float32(-0.25)
    up = tiny
    for _ in range(4):
        lo, hi, up = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf)), np.nextafter(up, np.float32(np.inf))
        near += [lo, hi, up, -up]
    x = np.concatenate([[0.0], mags, -mags, np.linspace(-0.3, 0.05, 4000).astype(np.float32), np.asarray(near, np.float32)]).astype(np.float32)
    x = np.unique(x)
    assert np.all((x == 0) | (np.abs(x) >= tiny)) and np.all(np.isfinite(x))
    pad = (-len(x)) % 16
    return np.concatenate([x, np.zeros(pad, np.float32)])                           # whole rows of the 16-wide identity network


def activation_reference(act, x):
    """(float64 act(x), yardstick = torch fp32 on the CPU against it, bar = 4 x max(yardstick, 2**-24))."""
    want = po._ACT[act](np.asarray(x, np.float64))
    yardstick = float(np.abs(_TORCH_ACT[act](torch.from_numpy(np.asarray(x, np.float32))).double().numpy() - want).max())
    return want, yardstick, 4.0 * max(yardstick, 2.0 ** -24)


# ------------------------------------------------------------------------------------------------ compute_returns
GAE_SHAPES = ((1, 2), (3, 255), (5, 257), (24, 1), (2, 1025))
GAE_DONES = ("none", "all", "random", "last")


def gae_inputs(T, n, dones):
    """(rewards, dones, values (T, n), last_values (n)): randn as in tests/test_hip_policy.py."""
    g = torch.Generator().manual_seed(1000 * T + n)
    r, v, last = torch.randn(T, n, generator=g), torch.randn(T, n, generator=g), torch.randn(n, generator=g)
    u = torch.rand(T, n, generator=g)
    d = torch.zeros(T, n)
    if dones == "all":
        d[:] = 1.0
    elif dones == "random":
        d = (u < 0.3).float()
    elif dones == "last":
        d[-1] = 1.0
    else:
        assert dones == "none"
    return r, d, v, last
