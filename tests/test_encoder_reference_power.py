"""CPU: can the per-stage sweep of the depth encoder (tests/test_hip_encoder_stages.py) see a fault?  No kernel runs here: the float64 torch
reference of `tools/train_estimator.TerrainEstimatorTorch`, on the sweep's own inputs and weights, is broken on purpose in the ways a tiled
implicit-GEMM kernel goes wrong, and every fault must move the output of the stage where it first acts by at least POWER = 10 bars of that stage
(bar_k = max(2e-5, 4 x the fp32-vs-float64 gap at stage k), the sweep's own rule).  These are conditions on the inputs: an input that fails them is
changed, the factor stays.  The same file keeps on record why the sweep is per stage: a dropped tap that moves a map by thousands of bars can
move the encoder's final features by less than one.

A tap "not read" is a zero in its place, so a fault on the input side is the true layer on an input with those entries zeroed.  A (fault, shape)
pair is left out only by a rule stated with the fault (`applies`): where the broken operation IS the true one (flooring a window end on a side
that divides by 4), or where the entry does not exist (no interior in a map under 3 on a side, no second env, no column >= 64).

This file also owns what both files share: the shapes, the two inputs, the weights and the bar."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from train_estimator import ENCODER_STAGE_ENDS, TerrainEstimatorTorch, closed_form_depth, closed_form_state, encoder_stages  # noqa: E402

FLOOR, POWER = 2e-5, 10.0
P, R = 6, 81
SHAPES = [(8, 8), (8, 128), (128, 8), (9, 11), (20, 24), (29, 57), (31, 33), (28, 56), (58, 87), (127, 128), (128, 128)]
CONV = ((5, 2, 2), (3, 2, 1), (3, 2, 1), (3, 1, 1))          # kernel, stride, padding
STAGE_NAMES = ("conv 1", "conv 2", "conv 3", "conv 4", "pool + flatten", "linear 1", "linear 2")


def conv4_side(side):
    for k, s, p in CONV:
        side = (side + 2 * p - k) // s + 1
    return side


def camera_input(n, shape):
    """The camera's real range, both signs: closed_form_depth - 0.5, in about +-0.5."""
    return closed_form_depth(1, n, *shape)[0] - 0.5


def wide_input(n, shape):
    """About +-3: the negative branches of ELU and tanh carry weight at conv 1."""
    return 6.0 * camera_input(n, shape)


def model_pair(shape, salt=0, out_dim=64, act="elu", default_init=False, **kw):
    """(fp32, float64) modules with `closed_form_state(salt)` weights, or torch's default initialisation seeded by `salt`."""
    torch.manual_seed(salt)
    m32 = TerrainEstimatorTorch(shape, kw.pop("proprio_dim", P), R, encoder_output_dim=out_dim, activation=act, **kw)
    if not default_init:
        m32.load_state_dict(closed_form_state(m32, salt=salt))
    return m32, copy.deepcopy(m32).double()


def stage_bars(m32, m64, x):
    """(float64 stage outputs, fp32-vs-float64 gap per stage, bar per stage)."""
    s64, s32 = encoder_stages(m64, x.double()), encoder_stages(m32, x)
    gaps = [float((a.double() - b).abs().max()) for a, b in zip(s32, s64)]
    return s64, gaps, [max(FLOOR, 4.0 * g) for g in gaps]


# ------------------------------------------------------------------------------------------------------------ the faults
def run_stage(m64, k, x, bias_mod=False, pool_floor=False, pixel_major=False):
    """Stage k (1..7) of the float64 module on stage k - 1's output `x`, optionally broken."""
    enc = m64.depth_encoder
    first = 0 if k == 1 else ENCODER_STAGE_ENDS[k - 2]
    layer, act = enc[first], enc[1]
    if k == 5:
        if pool_floor:
            n, c, h, w = x.shape
            y = torch.zeros(n, c, 4, 4, dtype=x.dtype)
            for i in range(4):
                for j in range(4):
                    win = x[:, :, (i * h) // 4:((i + 1) * h) // 4, (j * w) // 4:((j + 1) * w) // 4]
                    if win.numel():
                        y[:, :, i, j] = win.mean(dim=(2, 3))
        else:
            y = F.adaptive_avg_pool2d(x, (4, 4))
        return y.permute(0, 2, 3, 1).flatten(1) if pixel_major else y.flatten(1)
    b = layer.bias
    if bias_mod:
        b = b[torch.arange(b.numel()) % 64]
    if k <= 4:
        return act(F.conv2d(x, layer.weight, b, stride=layer.stride, padding=layer.padding))
    return act(F.linear(x, layer.weight, b))


def finish(m64, k, y):
    """The encoder's features from stage k's output."""
    for layer in m64.depth_encoder[ENCODER_STAGE_ENDS[k - 1]:]:
        y = layer(y)
    return y


def faults(out_dim):
    """(name, stage where it first acts, applies(input of that stage, n) -> bool, faulty stage output from (m64, that input))."""
    def zeroed(k, edit):
        def go(m64, x):
            x = x.clone()
            edit(x)
            return run_stage(m64, k, x)
        return go

    def strongest(x, y, xx):          # one entry of pixel (y, x) of env 0: the channel that carries most there (a real fault drops all of them)
        x[0, int(x[0, :, y, xx].abs().argmax()), y, xx] = 0.0

    def interior(x):
        strongest(x, x.shape[2] // 2, x.shape[3] // 2)

    def last_row(x):
        x[:, :, -1, :] = 0.0

    def last_col(x):
        x[:, :, :, -1] = 0.0

    def corner(x):
        strongest(x, 0, 0)

    def aliased(k):
        def go(m64, x):
            y = run_stage(m64, k, x).clone()
            y[1] = y[0]
            return y
        return go

    always = lambda x, n: True                                             # noqa: E731
    out = []
    for l in range(1, 5):
        out.append((f"last input row not read at conv {l}", l, always, zeroed(l, last_row)))
        out.append((f"last input column not read at conv {l}", l, always, zeroed(l, last_col)))
        out.append((f"corner entry not read at conv {l}", l, always, zeroed(l, corner)))
        # an interior entry exists only in a map of 3 or more on both sides
        out.append((f"interior entry of env 0 not read at conv {l}", l, lambda x, n: min(x.shape[2:]) >= 3, zeroed(l, interior)))
    # flooring the window end is the identity on a side that divides by 4
    out.append(("pooling window end floored", 5, lambda x, n: x.shape[2] % 4 != 0 or x.shape[3] % 4 != 0, lambda m, x: run_stage(m, 5, x, pool_floor=True)))
    out.append(("flatten written pixel major", 5, always, lambda m, x: run_stage(m, 5, x, pixel_major=True)))
    # c % 64 is c below 64: the layers of more than 64 columns are conv 3, linear 1 and, for out_dim > 64, linear 2
    for k, width in ((3, 128), (6, 128), (7, out_dim)):
        out.append((f"bias of column c taken from c % 64 at {STAGE_NAMES[k - 1]}", k, lambda x, n, width=width: width > 64,
                    lambda m, x, k=k: run_stage(m, k, x, bias_mod=True)))
    for k in range(1, 8):
        out.append((f"rows of the second env taken from the first at {STAGE_NAMES[k - 1]}", k, lambda x, n: n >= 2, aliased(k)))
    return out


CASES = [(s, 64, "camera", False) for s in SHAPES] + [((29, 57), 65, "camera", False), ((28, 56), 65, "camera", False), ((29, 57), 64, "wide", False),
                                                       ((28, 56), 64, "wide", False), ((29, 57), 64, "camera", True)]


def reference_case(shape, out_dim=64, kind="camera", default_init=False, n=3):
    """(float64 module, input of every stage, float64 stage outputs, gaps, bars) of one case."""
    m32, m64 = model_pair(shape, salt=SHAPES.index(shape), out_dim=out_dim, default_init=default_init)
    x = (camera_input if kind == "camera" else wide_input)(n, shape)
    s64, gaps, bars = stage_bars(m32, m64, x)
    return m64, [x.double().unsqueeze(1)] + s64[:-1], s64, gaps, bars


@pytest.mark.parametrize("shape,out_dim,kind,default_init", CASES, ids=[f"{s[0]}x{s[1]}-{o}-{k}{'-default' if d else ''}" for s, o, k, d in CASES])
def test_every_fault_moves_its_stage_by_ten_bars(shape, out_dim, kind, default_init):
    n = 3
    m64, inputs, s64, gaps, bars = reference_case(shape, out_dim, kind, default_init, n)
    seen = 0
    for name, k, applies, broken in faults(out_dim):
        if not applies(inputs[k - 1], n):
            continue
        with torch.no_grad():
            moved = float((broken(m64, inputs[k - 1]) - s64[k - 1]).abs().max())
        print(f"{shape} {name}: stage {k} moved {moved:.3e} = {moved / bars[k - 1]:.0f} bars (gap {gaps[k - 1]:.3e}, bar {bars[k - 1]:.3e})")
        assert moved >= POWER * bars[k - 1], (shape, name, k, moved, bars[k - 1])
        seen += 1
    assert seen >= 20


def test_the_end_to_end_check_alone_misses_a_dropped_tap():
    """Why the sweep is per stage: behind AdaptiveAvgPool2d and two linear layers, an interior entry that a convolution does not read -- at least ten
    bars at its own stage, asserted above and again here -- moves the final features by less than the end-to-end bar at the larger images."""
    hidden = []
    for shape in ((58, 87), (127, 128), (128, 128)):
        m64, inputs, s64, gaps, bars = reference_case(shape)
        for name, k, applies, broken in faults(64):
            if "interior" not in name:
                continue
            with torch.no_grad():
                y = broken(m64, inputs[k - 1])
                own, end = float((y - s64[k - 1]).abs().max()), float((finish(m64, k, y) - s64[-1]).abs().max())
            print(f"{shape} {name}: its own stage moved {own / bars[k - 1]:.0f} bars, the final features {end:.3e} (end-to-end bar {bars[-1]:.3e})")
            assert own >= POWER * bars[k - 1]
            if end < bars[-1]:
                hidden.append((shape, name, end))
    assert hidden, "no dropped tap stays under the end-to-end bar any more: the record in this docstring is out of date"


def test_the_shape_list_covers_the_pooling_regimes():
    sides = {conv4_side(v) for s in SHAPES for v in s}
    assert {1, 2, 3} <= sides and any(v >= 4 and v % 4 for v in sides) and any(v % 4 == 0 for v in sides), sides
    assert {s % 2 for sh in SHAPES for s in sh} == {0, 1}
    assert np.all(np.array(SHAPES) >= 8) and np.all(np.array(SHAPES) <= 128)
