"""Holds tests/distill_reference.py (the float64 / float32 torch restatement the GPU tests use) to tests/golden/distillation_update.npz, that is,
to the reference's own `Distillation.update` run on torch-CPU: the loss, the parameters, the untouched teacher and std.  Also asserts, on the
reference alone in float64, the conditions the GPU tests rely on: the Huber rows sit on both sides of the kink and clear of it, and the clip test's
two `max_grad_norm` values bracket the group's norm.  No GPU needed."""
import ctypes as C
import os

import pytest
import torch

from tests import distill_reference as ref

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "extended_legged_gym_amd", "csrc", "liblgstep.so")


def _slab():
    from extended_legged_gym_amd import abi
    return int(abi.declare_train(C.CDLL(LIB)).lg_ppo_wgrad_slab_rows())


def _run(case, dtype):
    return ref.update(case["sd0"], case["activation"], case["observations"], case["privileged_actions"], dtype=dtype, **case["alg"])


@pytest.mark.parametrize("name", ["g_mse", "g_huber"])
def test_restatement_reproduces_the_references_update(name):
    case = ref.load_golden_case(name)
    T, G, E = case["T"], case["alg"]["gradient_length"], case["alg"]["num_learning_epochs"]
    p32, loss32, trace32 = _run(case, torch.float32)
    p64, loss64, trace64 = _run(case, torch.float64)
    assert len(trace64["step_losses"]) == E * T and len(trace64["norms"]) == (E * T) // G and len(trace64["rest_diffs"]) == (E * T) % G
    assert trace64["state"]["step"] == (E * T) // G
    want = case["loss"]
    print(name, "loss fp32", loss32["behavior"], "float64", loss64["behavior"], "reference", want)
    assert abs(loss32["behavior"] - want) <= 2e-6 * abs(want)
    assert abs(loss64["behavior"] - want) <= 1e-5 * abs(want)
    moved = case["alg"]["learning_rate"] * ((E * T) // G)          # the sum of the optimiser steps' learning rates
    for k, w in case["sd1"].items():
        if k.startswith("student."):
            scale = float(w.abs().max())
            assert float((p32[k] - w).abs().max()) <= 0.02 * moved + 1e-6 * scale, k
            assert float((p64[k].float() - w).abs().max()) <= 0.10 * moved + 1e-6 * scale, k
            assert not torch.equal(w, case["sd0"][k]), k
        else:          # only the student moves: the reference's own update and the restatement both leave these bits alone
            assert torch.equal(w, case["sd0"][k]) and torch.equal(p32[k], case["sd0"][k]) and torch.equal(p64[k], case["sd0"][k]), k


def test_golden_huber_rows_sit_on_both_sides_of_the_kink():
    case = ref.load_golden_case("g_huber")
    assert case["alg"]["loss_type"] == "huber" and not case["alg"]["max_grad_norm"]
    _, _, trace = _run(case, torch.float64)
    assert len(trace["group_diffs"]) == 2 and len(trace["rest_diffs"]) == 2          # the second group wraps the epoch boundary
    for d in trace["group_diffs"]:
        above, below, clear = ref.huber_fractions(d)
        print("g_huber group", above, below, clear)
        assert above >= 0.10 and below >= 0.10 and clear >= 1e-4


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_crafted_huber_rows_sit_on_both_sides_of_the_kink(shape):
    sd, act, N, G = ref.shape_case(shape, _slab())
    rows = ref.craft_rows(sd, act, G, N, ref.GROUP_SEED)
    _, _, _, diffs = ref.group_gradients(sd, act, rows["observations"], rows["privileged_actions"], 0, G, "huber", torch.float64)
    above, below, clear = ref.huber_fractions(torch.stack(diffs))
    print(shape, above, below, clear)
    assert above >= 0.10 and below >= 0.10 and clear >= 1e-4


def test_clip_values_bracket_the_groups_norm():
    sd, act, N, G = ref.shape_case("D1", _slab())
    rows = ref.craft_rows(sd, act, G, N, ref.GROUP_SEED, spread=ref.OPT_SPREAD)
    _, norm, _, _ = ref.group_gradients(sd, act, rows["observations"], rows["privileged_actions"], 0, G, "mse", torch.float64)
    print("norm", float(norm))
    assert ref.CLIP_SMALL < float(norm) < ref.CLIP_LARGE
    assert float(norm) > 2.0          # "well above 1": an unclipped step and one clipped at 1 differ by more than a factor of two
