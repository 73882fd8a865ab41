"""CPU checks of tests/estimator_update_reference.py, the float64 reference tests/test_hip_estimator_update.py holds the kernels to.

Conditions on the inputs: every tensor has a gradient on every case; the Huber cases have at least 10 % of their elements on each side of the kink and
none within 1e-4 of it; the l1 cases have no |diff| < 1e-4; the clip values of the optimiser test bracket the group's norm.

Power, in the manner of tests/test_encoder_reference_power.py: the float64 reference is broken in the ways these kernels can go wrong, and each fault
must move at least one checked figure by POWER = 10 bars (bar = max(8 e32, 2e-5), e32 from torch's fp32 run of the same case) on at least one of
the GPU test's cases.  A per-pixel fault in a weight gradient is diluted by the row count, so the case list holds (8, 8) and (9, 11) at N = 1 .. 3."""
import functools

import pytest
import torch

from tests import estimator_update_reference as ref
from tests.test_encoder_reference_power import POWER


def _cases():
    return ref.group_cases() + [ref.slab_case(64)]          # the slab case at a stand-in slab size: its inputs are built the same way


@functools.lru_cache(maxsize=None)
def _clean(i):
    case = _cases()[i]
    ud, carry = bool(case.dones_at), ref.carry_of(case)
    g64, n64, l64, _, _ = ref.group_gradients(case, torch.float64, carry=carry, use_dones=ud)
    g32, n32, l32, _, _ = ref.group_gradients(case, torch.float32, carry=carry, use_dones=ud)
    return case, g64, {k: ref.bar(ref.err(g32[k], g64[k])) for k in g64}


@pytest.mark.parametrize("i", range(len(_cases())), ids=[c.name for c in _cases()])
def test_inputs_meet_their_conditions(i):
    case, g64, bars = _clean(i)
    for k, g in g64.items():
        assert float(g.abs().max()) > 0, (case.name, k)
    print(case.name, "largest bar", max(bars.values()))
    if case.loss == "mse":
        return
    model, rows, st = case.module(torch.float64), ref.to_dtype(case.rows(), torch.float64), ref.cast(ref.carry_of(case), torch.float64)
    diffs = []
    with torch.no_grad():
        for t in range(case.G):
            pred, st = ref.step(model, case, rows, t, st)
            diffs.append((pred - rows["raycast_targets"][t]).abs().flatten())
    d = torch.cat(diffs)
    if case.loss == "huber":
        below, above = float((d < 1).double().mean()), float((d > 1).double().mean())
        print(case.name, "below the kink", below, "above", above, "closest", float((d - 1).abs().min()))
        assert below >= 0.1 and above >= 0.1 and float((d - 1).abs().min()) >= 1e-4
    else:
        print(case.name, "smallest |diff|", float(d.min()))
        assert float(d.min()) >= 1e-4


def test_clip_values_bracket_the_norm():
    case = ref.Case(**ref.OPT_CASE)
    _, norm, _, _, _ = ref.group_gradients(case, torch.float64)
    print("norm", norm)
    assert ref.CLIP_SMALL < norm < ref.CLIP_LARGE


GROUP_FAULTS = [("drop_last_pixel", 1), ("drop_last_pixel", 2), ("drop_last_pixel", 3), ("drop_last_pixel", 4), ("parity", 2), ("parity", 3),
                ("tap_transposed", 2), ("tap_transposed", 3), ("tap_transposed", 4), ("pool_floor", True), ("act_negative", True),
                ("slab_tail", 1), ("slab_tail", 2), ("slab_tail", 3), ("slab_tail", 4), ("bias_high", 3), ("bptt_cut", True)]


@pytest.mark.parametrize("fault,value", GROUP_FAULTS, ids=[f"{f}-{v}" for f, v in GROUP_FAULTS])
def test_the_bar_sees_a_broken_backward_pass(fault, value):
    """At least one tensor's gradient moves by >= POWER bars on at least one case."""
    best = (0.0, None, None)
    for i in range(len(_cases())):
        case, g64, bars = _clean(i)
        if fault == "act_negative" and case.act == "relu":
            continue          # ReLU's negative branch IS 0
        if fault == "bptt_cut" and case.G < 2:
            continue
        gf, _, _, _, _ = ref.group_gradients(case, torch.float64, carry=ref.carry_of(case), use_dones=bool(case.dones_at), faults={fault: value})
        for k in g64:
            moved = ref.err(gf[k], g64[k]) / bars[k]
            if moved > best[0]:
                best = (moved, case.name, k)
        if best[0] >= POWER:
            break
    print(f"{fault} {value}: moved {best[2]} of {best[1]} by {best[0]:.1f} bars")
    assert best[0] >= POWER, best


def test_the_bar_sees_a_chain_not_cut_at_a_groups_first_step():
    """The second group of the update case (steps 3, 0, 1 after steps 0, 1, 2): its first step's entering state left attached to the steps before."""
    case = ref.Case(**ref.UPDATE_CASE)
    kw = dict(first_step=3, num_steps=3, pre_steps=3)
    g64, g32 = ref.group_gradients(case, torch.float64, **kw)[0], ref.group_gradients(case, torch.float32, **kw)[0]
    bad = ref.group_gradients(case, torch.float64, faults={"no_detach": True}, **kw)[0]
    moved = {k: ref.err(bad[k], g64[k]) / ref.bar(ref.err(g32[k], g64[k])) for k in g64}
    k = max(moved, key=moved.get)
    print("no_detach moved", k, "by", moved[k], "bars")
    assert moved[k] >= POWER


def test_the_bar_sees_an_epoch_seeded_from_the_previous_epochs_end():
    """The step losses of the second epoch move by >= POWER bars of what tests/test_hip_estimator_update.py checks on the whole update."""
    fault = "epoch_chain"
    case = ref.Case(**ref.UPDATE_CASE)
    kw = dict(E=2, lr=2e-3, max_grad_norm=1.0)
    r64, r32, bad = ref.run_update(case, torch.float64, **kw), ref.run_update(case, torch.float32, **kw), ref.run_update(case, torch.float64, faults={fault: True}, **kw)
    rel = lambda a, b: abs(a - b) / abs(b)          # noqa: E731
    moved = [rel(bad["grad_norm"], r64["grad_norm"]) / ref.bar(rel(r32["grad_norm"], r64["grad_norm"]))]
    moved += [rel(b, w) / ref.bar(rel(s, w)) for b, s, w in zip(bad["losses"], r32["losses"], r64["losses"])]
    print(fault, "moved a checked figure by", max(moved), "bars")
    assert max(moved) >= POWER


@pytest.mark.parametrize("name", sorted(ref.GOLDEN_CASES))
def test_the_restatement_is_the_references_update(name):
    """tests/golden/estimator_update.npz holds what the reference's `EstimatorDistillation.update` gave in float64; the restatement gives the same."""
    spec, want = ref.GOLDEN_CASES[name], ref.golden(name)["f64"]
    case = ref.Case(**spec["case"])
    got = ref.run_update(case, torch.float64, E=spec["E"], lr=spec["lr"], max_grad_norm=spec["max_grad_norm"])
    assert len(got["losses"]) == len(want["step_losses"])
    assert max(abs(a - b) / abs(b) for a, b in zip(got["losses"], want["step_losses"])) < 1e-11
    assert abs(got["mean"] - float(want["loss"])) / float(want["loss"]) < 1e-11 and abs(got["grad_norm"] - float(want["grad_norm"])) / float(want["grad_norm"]) < 1e-11
    assert ref.err(ref.predict(got["model"], case, case.rows(), t=1), torch.from_numpy(want["probe"])) < 1e-11
    norms = [float(v.double().norm()) for v in got["model"].state_dict().values()]
    assert max(abs(a - b) / b for a, b in zip(norms, want["norms"])) < 1e-11
