"""The backward kernels of the bf16 trainer (csrc/lg_estimator_train_bf16.hip) stage by stage, through `lg_estimator_bf16train_backward_stage`: the
production kernels and grids on the trainer's own saved rows.

After one forward group the chain is walked backwards from a seeded delta w.r.t. the pre-activation of linear 2.  Each stage gets the PREVIOUS stage's
native output as its delta and the trainer's own `saved_stage` rows as operands, so one rounding flip cannot spread; it is compared with float64 on
those same operands (tests/estimator_bf16_update_rule.py `stage_backward`).

    outputs stored as bf16 (pool backward, the data gradients of conv 4 / 3 / 2): every entry inside [R(u - bar), R(u + bar)], bar = max(FLOOR, 4 gap),
        gap = torch fp32 against float64 for that stage on those operands: the rule and FLOOR of tests/bf16_encoder_rule.py;
    fp32 outputs (dW, db, the linear layers' deltas): e <= max(8 e32, 2e-5), the bar of tests/test_hip_estimator_update.py, e32 torch fp32 on those
        operands.

tests/test_estimator_bf16_update_rule.py shows, without a GPU, that these bars see every fault of tests/estimator_update_reference.py that applies to
a stage.  Every figure is printed before it is asserted."""
import pytest
import torch

from tests import estimator_bf16_update_rule as rule
from tests import estimator_update_reference as ref
from tests.bf16_encoder_rule import FLOOR, R, check_interval

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _slab():
    from extended_legged_gym_amd import abi
    from extended_legged_gym_amd.rl.estimator_distillation import _estimator_train_lib
    return int(abi.declare(_estimator_train_lib(), "estimator_train_bf16").lg_estimator_bf16train_wgrad_slab_rows())


def _cases():
    return [
        ref.Case("8x8_n1", (8, 8), 1, 1),
        ref.Case("9x11_n3", (9, 11), 3, 1, salt=1),
        ref.Case("8x128_n3_relu", (8, 128), 3, 1, act="relu", salt=2),
        ref.Case("128x8_n3_tanh", (128, 8), 3, 1, act="tanh", salt=3),
        ref.Case("29x57_n3_f40", (29, 57), 3, 1, F=40, salt=4),
        ref.Case("28x56_n70_g2", (28, 56), 70, 2, salt=7),
        ref.slab_case(8192),          # rebuilt from the library's slab size in the test
    ]


def _maps(t):
    """(rows, y, x, channel) of the kernels -> torch's (rows, channel, y, x)."""
    return t.permute(0, 3, 1, 2).contiguous()


def _rows_last(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _fp32_ok(tag, got, want, got32):
    e, e32 = ref.err(got, want), ref.err(got32, want)
    bar = ref.bar(e32)
    print(f"{tag}: e {e:.3e}  e32 {e32:.3e}  bar {bar:.3e}")
    return e <= bar


def _interval_ok(tag, got, u, u32, k):
    gap = float((u32.double() - u).abs().max())
    try:
        check_interval(tag, got, u, max(FLOOR, 4.0 * gap), gap, k)
        return True
    except AssertionError as e:
        print(e)
        return False


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c.name)
def test_backward_stages_on_the_trainers_own_rows(case):
    from extended_legged_gym_amd.rl import NativeEstimatorDistillation, NativeTerrainEstimator
    if case.name == "9x11_slabs":
        case = ref.slab_case(_slab())
        assert case.N % 2 == 1 and (case.N * 4) % _slab() % 8 != 0          # conv 3 / conv 4: two full slabs and a ragged third, not a multiple of 8 rows
    state, rows = case.state(), case.rows()
    est = NativeTerrainEstimator(state, case.shape, case.P, activation=case.act, memory_type=case.memory, device=DEV, encoder_precision="bf16")
    alg = NativeEstimatorDistillation(est, state, gradient_length=case.G, loss_type=case.loss, encoder_training="bf16")
    crows = {k: v.to(DEV) for k, v in rows.items()}          # kept to the end: the weight gradient of conv 1 reads the group call's images
    alg.group(crows, 0, case.G, train=False)
    n, act = case.G * case.N, case.act
    image = R(rows["depth_images"][:case.G].reshape(n, 1, *case.shape))
    saved = {k: alg.saved_stage(k).cpu() for k in range(1, 7)}
    y = {k: _maps(saved[k]) for k in range(1, 5)}          # stored outputs of conv 1-4
    pool, y5 = saved[5], saved[6]
    for t in saved.values():          # what is saved is bf16
        assert torch.equal(R(t), t)
    W = {i: R(state[f"depth_encoder.{i}.weight"]) for i in (0, 2, 4, 6, 10, 12)}
    g = torch.Generator().manual_seed(31 + case.salt)
    ok = True

    def dense(tag, stage, delta, x, w, y_below, out_width):
        got_dx, (got_dw, got_db) = alg.backward_stage(stage, delta, (n, out_width), tuple(w.shape))
        want = rule.stage_backward("linear", act, delta, x=x, w=w, y_below=y_below)
        w32 = rule.stage_backward32("linear", act, delta, x=x, w=w, y_below=y_below)
        good = True
        for name, a, b, c in zip(("dX", "dW", "db"), (got_dx, got_dw, got_db), want, w32):
            good &= _fp32_ok(f"{case.name} {tag} {name}", a.cpu(), b, c)
        return good, got_dx.cpu()

    d6 = torch.randn(n, case.F, generator=g)
    good, d5 = dense("linear 2", "linear2", d6, y5, W[12], y5, 128)
    ok &= good
    good, dpool = dense("linear 1", "linear1", d5, pool, W[10], None, 1024)
    ok &= good
    # pool backward: stored bf16
    got, _ = alg.backward_stage("pool_backward", dpool, tuple(saved[4].shape))
    delta = _maps(got.cpu())
    assert torch.equal(R(delta), delta)
    ok &= _interval_ok(f"{case.name} pool backward", delta, rule.stage_backward("pool", act, dpool, y_below=y[4]), rule.stage_backward32("pool", act, dpool, y_below=y[4]), 4)
    # conv 4 .. conv 1: the weight gradient on the delta that stands, then the data gradient into the layer below
    for l, i, (stride, pad) in reversed(list(zip((1, 2, 3, 4), ref.CONV_INDEX, rule.CONV_SHAPES))):
        x = image if l == 1 else y[l - 1]
        _, (got_dw, got_db) = alg.backward_stage(f"wgrad_conv{l}", _rows_last(delta), None, tuple(W[i].shape))
        want = rule.stage_backward("conv", act, delta, x=x, w=W[i], y_below=None, stride=stride, pad=pad)
        w32 = rule.stage_backward32("conv", act, delta, x=x, w=W[i], y_below=None, stride=stride, pad=pad)
        ok &= _fp32_ok(f"{case.name} conv {l} dW", got_dw.cpu(), want[1], w32[1])
        ok &= _fp32_ok(f"{case.name} conv {l} db", got_db.cpu(), want[2], w32[2])
        if l == 1:
            break
        got, _ = alg.backward_stage(f"dgrad_conv{l}", _rows_last(delta), tuple(saved[l - 1].shape))
        below = _maps(got.cpu())
        assert torch.equal(R(below), below)
        u = rule.stage_backward("conv", act, delta, x=x, w=W[i], y_below=x, stride=stride, pad=pad)[0]
        u32 = rule.stage_backward32("conv", act, delta, x=x, w=W[i], y_below=x, stride=stride, pad=pad)[0]
        ok &= _interval_ok(f"{case.name} conv {l} data gradient", below, u, u32, l - 1)
        delta = below
    alg.close(); est.close()
    del crows
    assert ok
