"""CPU: can tests/test_hip_wide_input.py see a slab of the split-K first layer go wrong?  No kernel runs here.  On the GPU test's own shapes, weights
and rows (tests/wide_input.py, tests/policy_sweep.py) the float64 reference is evaluated with ONE layer-0 input column read as zero -- what a slab
staged at the wrong offset, a block skipped at a slab edge or a weight pointer one block off does to a column -- and the output must move by at least
POWER = 10 bars (bar = max(2e-5, 4 x the fp32-vs-float64 yardstick), the sweep's rule).  `policy_sweep.case` asserts for every network that the 2e-5
floor binds and that the outputs are O(1).  These are conditions on the inputs: a later change of them that blunts the GPU test fails here."""
import numpy as np
import pytest

from oracle import policy_oracle as po
from tests import policy_sweep as ps
from tests import wide_input as wi


@pytest.mark.parametrize("dims,act", wi.FORWARD_CASES, ids=[ps.case_id(d, a) for d, a in wi.FORWARD_CASES])
def test_a_layer0_column_read_as_zero_moves_the_output_by_ten_bars(dims, act):
    layers, x, want, yardstick, bar = ps.case(dims, act)
    assert bar == ps.FLOOR and 0.05 <= float(np.abs(want).max()) <= 20.0
    x = x.numpy()
    worst = None
    for k in wi.columns_of(dims[0]):
        broken = x.copy()
        broken[:, k] = 0.0
        moved = float(np.abs(po.mlp_forward(layers, broken, act) - want).max())
        print(f"{ps.case_id(dims, act)} column {k} (slab {k // wi.SLAB}) read as zero: moved {moved:.3e} = {moved / bar:.0f} bars (yardstick {yardstick:.3e})")
        assert moved >= ps.POWER * bar, (dims, act, k, moved, bar)
        worst = moved if worst is None else min(worst, moved)
    print(f"{ps.case_id(dims, act)}: the weakest column at {worst / bar:.0f} bars")


def test_act_pairs_have_o1_outputs_under_the_floor():
    for salt, (adims, cdims) in enumerate(wi.ACT_PAIRS):
        for dims in (adims, cdims, ps.teacher_dims(cdims, adims[-1])):
            _, _, want, yardstick, bar = ps.case(dims, "elu", salt=20 + salt)
            print(f"{dims}: yardstick {yardstick:.3e}, bar {bar:.3e}, max |y| {float(np.abs(want).max()):.3f}")
            assert bar == ps.FLOOR


def test_the_shape_list_reaches_every_slab_path():
    firsts = {d[0] for d in wi.DIMS}
    assert {513, 577, 578, 1023, 1024, 1025, 1536, 2047, 2048} == firsts and all(wi.SLAB < k <= 2048 for k in firsts)
    assert {-(-k // wi.SLAB) for k in firsts} == {2, 3, 4}                                   # slab counts
    assert any(k % wi.SLAB == 0 for k in firsts) and any(((k + 63) & ~63) % wi.SLAB == 64 for k in firsts)      # a full last slab, and one of a single block
    assert all(1 <= w <= 512 for d in wi.DIMS for w in d[1:])
    chunks = {(d[1] + 15) // 16 if len(d) == 2 else ((d[1] + 63) & ~63) // 16 for d in wi.DIMS}
    assert {1, 4, 8, 32} <= chunks, chunks          # one wave busy, half the waves, one chunk per wave, four per wave
    assert {len(d) - 1 for d in wi.DIMS} >= {1, 2, 4}
    wide = [[a[0] > wi.SLAB, c[0] > wi.SLAB] for a, c in wi.ACT_PAIRS]
    assert [True, True] in wide and [True, False] in wide and [False, True] in wide
