"""What the GPU tests of the bf16 trainer can see (tests/test_hip_estimator_bf16_update.py, tests/test_hip_estimator_bf16_stages.py), shown on the CPU
with tests/estimator_bf16_update_rule.py.  No GPU needed.

(a) A trainer that differentiates the wrong function is seen: on the group cases (all but the registered one, see below) the plain float64 gradient (no rounding anywhere) differs from the
    float64 rule reference, in its worst tensor, by more than that tensor's bar max(4 y, 2e-5), y the fp32 emulation's error.
(b) The stage bars have power: on operands whose values are bf16-representable, every fault of tests/estimator_update_reference.py that applies to a
    stage's dX, dW or db moves that output beyond the stage's bar -- for fp32 outputs max(8 e32, 2e-5) by at least POWER, for outputs stored as bf16
    out of the interval [R(u - bar), R(u + bar)] and by at least POWER bars.  `bias_high` applies to conv 3 only (the one with more than 64 output
    channels), `parity` to the stride-2 layers only."""
import pytest
import torch

from tests import estimator_bf16_update_rule as rule
from tests import estimator_update_reference as ref
from tests.bf16_encoder_rule import FLOOR, R, outside

POWER = 10.0          # tests/test_encoder_reference_power.py's margin
CHANNELS = {2: (32, 64), 3: (64, 128), 4: (128, 64)}          # conv l: C_in, C_out


# every group case but the registered 28 x 56 x 70 x 15 one: its three CPU passes over 1050 rows take minutes, and part (a) does not cover it
@pytest.mark.parametrize("case", [c for c in ref.group_cases() if c.N * c.G <= 210], ids=lambda c: c.name)
def test_the_plain_gradient_lies_outside_the_rules_bar(case):
    use_dones, carry = bool(case.dones_at), ref.carry_of(case)
    g64, *_ = rule.group_gradients(case, torch.float64, carry=carry, use_dones=use_dones)
    g32, *_ = rule.group_gradients(case, torch.float32, round_deltas=True, carry=carry, use_dones=use_dones)
    plain, *_ = ref.group_gradients(case, torch.float64, carry=carry, use_dones=use_dones)
    worst = 0.0
    for k in g64:
        y, e = ref.err(g32[k], g64[k]), ref.err(plain[k], g64[k])
        bar = max(4.0 * y, 2e-5)
        print(f"{case.name} {k}: plain against the rule {e:.3e}  y {y:.3e}  bar {bar:.3e}")
        worst = max(worst, e / bar)
    assert worst > 1.0


def _side(v, k, s, p):
    return (v + 2 * p - k) // s + 1


def _operands(l, image, n=3, seed=0):
    """bf16-representable operands of conv l = 2..4 for an image of that size: x the stored ELU output below, w, and a delta on the layer's output."""
    h, w = image
    for (k, s, p) in ((5, 2, 2), (3, 2, 1), (3, 2, 1))[:l - 1]:
        h, w = _side(h, k, s, p), _side(w, k, s, p)
    stride, pad = rule.CONV_SHAPES[l - 1]
    ho, wo = _side(h, 3, stride, pad), _side(w, 3, stride, pad)
    cin, cout = CHANNELS[l]
    g = torch.Generator().manual_seed(100 * l + seed)
    x = R(torch.nn.functional.elu(torch.randn(n, cin, h, w, generator=g)))
    wt = R(0.1 * torch.randn(cout, cin, 3, 3, generator=g))
    d = R(torch.randn(n, cout, ho, wo, generator=g))
    return x, wt, d, stride, pad


def _fp32_power(tag, faulty, clean, c32):
    e, bar = ref.err(faulty, clean), ref.bar(ref.err(c32, clean))
    print(f"{tag}: fault {e:.3e}  bar {bar:.3e}  x{e / bar:.0f}")
    return e > POWER * bar


def _interval_power(tag, faulty, u, u32, k):
    gap = float((u32.double() - u).abs().max())
    bar = max(FLOOR, 4.0 * gap)
    out = int(outside(R(faulty), u, bar, k).sum())
    worst = float((faulty - u).abs().max())
    print(f"{tag}: {out} of {u.numel()} entries outside, max |fault| {worst:.3e}  bar {bar:.3e}  x{worst / bar:.0f}")
    return out > 0 and worst > POWER * bar


@pytest.mark.parametrize("image", [(9, 11), (15, 29)])
@pytest.mark.parametrize("l", [2, 3, 4])
def test_every_applicable_fault_exceeds_the_stage_bar(l, image):
    x, w, d, stride, pad = _operands(l, image)
    kw = dict(x=x, w=w, y_below=x, stride=stride, pad=pad)
    clean, c32 = rule.stage_backward("conv", "elu", d, **kw), rule.stage_backward32("conv", "elu", d, **kw)
    faults = {"drop_last_pixel": (0, 1, 2), "slab_tail": (1, 2), "tap_transposed": (0,), "act_negative": (0,)}
    if stride == 2:
        faults["parity"] = (0,)
    if w.shape[0] > 64:
        faults["bias_high"] = (2,)
    ok = True
    for name, outputs in faults.items():
        got = rule.stage_backward("conv", "elu", d, faults={name: l}, stage=l, **kw)
        for o in outputs:
            tag = f"conv {l} {image} {name} {('dX', 'dW', 'db')[o]}"
            ok &= _interval_power(tag, got[o], clean[o], c32[o], l - 1) if o == 0 else _fp32_power(tag, got[o], clean[o], c32[o])
    assert ok


@pytest.mark.parametrize("shape", [(2, 2), (3, 5), (4, 7)])          # conv 4's map of a 9 x 11 .. 28 x 56 image
def test_the_pooling_faults_exceed_the_stage_bar(shape):
    g = torch.Generator().manual_seed(5)
    y4 = R(torch.nn.functional.elu(torch.randn(3, 64, *shape, generator=g)))
    dp = torch.randn(3, 1024, generator=g)
    u, u32 = rule.stage_backward("pool", "elu", dp, y_below=y4), rule.stage_backward32("pool", "elu", dp, y_below=y4)
    ok = _interval_power(f"pool {shape} act_negative", rule.stage_backward("pool", "elu", dp, y_below=y4, faults={"act_negative": 1}), u, u32, 4)
    if any(s % 4 for s in shape) and max(shape) > 4:          # the floored window end differs from torch's only where a side is no multiple of 4 and windows overlap
        ok &= _interval_power(f"pool {shape} pool_floor", rule.stage_backward("pool", "elu", dp, y_below=y4, faults={"pool_floor": 1}), u, u32, 4)
    assert ok
