"""Holds tests/ppo_reference.py (the float64 / float32 torch restatement the GPU tests use) to tests/golden/ppo_update.npz, that is, to the
reference's own `PPO.update` run on torch-CPU: losses, learning rate, parameters.  Also asserts, on the reference alone, the conditions the GPU tests
rely on: every branch of the clipped losses is populated by the crafted rows, the adaptive cases keep the float64 KL 5 % away from both thresholds
at every mini-batch, and the learning rate moves both up and down.  No GPU needed."""
import pytest
import torch

from tests import ppo_reference as ref


def _run(case, dtype):
    kw = case["ppo"]
    hyper = {k: kw[k] for k in ref.HYPER}
    return ref.update(case["sd0"], case["activation"], case["rows"], case["perm"], hyper, kw["num_learning_epochs"], kw["num_mini_batches"],
                      kw["learning_rate"], dtype)


@pytest.mark.parametrize("name", ["mb1", "mb3"])
def test_restatement_reproduces_the_references_update(name):
    case = ref.load_golden_case(name)
    p32, loss32, lr32, trace32, _ = _run(case, torch.float32)
    p64, loss64, lr64, trace64, _ = _run(case, torch.float64)
    assert lr32 == case["learning_rate"] and lr64 == case["learning_rate"]
    assert [t["learning_rate"] for t in trace32] == case["lr_trajectory"] and [t["learning_rate"] for t in trace64] == case["lr_trajectory"]
    for k, want in case["loss"].items():
        # fp32 against the reference's fp32 run: the same arithmetic up to the order of a few sums; float64: the fp32 rounding of a mean of O(1) terms
        assert abs(loss32[k] - want) <= 2e-6 * abs(want), (k, loss32[k], want)
        assert abs(loss64[k] - want) <= 1e-5 * abs(want), (k, loss64[k], want)
    for k, want in case["sd1"].items():
        scale = float(want.abs().max())
        # an Adam step moves a parameter by about lr whatever the gradient's size, so a different rounding of a near-zero gradient shows up as a
        # fraction of lr: the fp32 restatement is held to 2 % of the total movement (the sum of the steps' learning rates), float64 to 10 %
        moved = sum(case["lr_trajectory"])
        assert float((p32[k] - want).abs().max()) <= 0.02 * moved + 1e-6 * scale, k
        assert float((p64[k].float() - want).abs().max()) <= 0.10 * moved + 1e-6 * scale, k
        assert float((p64[k].float() - want).abs().mean()) <= 1e-5 * max(scale, 1.0), k
    if name == "mb1":          # one mini-batch: the permutation only reorders a sum
        other = dict(case, perm=torch.arange(case["perm"].numel()))
        _, loss_id, _, _, _ = _run(other, torch.float64)
        for k in loss64:
            assert abs(loss_id[k] - loss64[k]) <= 1e-12 * abs(loss64[k])


@pytest.mark.parametrize("name", ["mb1", "mb3"])
def test_crafted_rows_populate_every_clip_branch(name):
    case = ref.load_golden_case(name)
    _, _, _, trace, _ = _run(case, torch.float64)
    kw = case["ppo"]
    mini = case["rows"]["observations"].shape[0] // kw["num_mini_batches"]
    for step, t in enumerate(trace):
        i = step % kw["num_mini_batches"]
        adv = case["rows"]["advantages"][case["perm"][i * mini:(i + 1) * mini], 0].double()
        frac = ref.branch_fractions(t["ratio"], t["dv"], adv, kw["clip_param"])
        assert min(frac[k] for k in frac if k.startswith(("pos", "neg"))) >= 0.05, (step, frac)
        assert min(frac["value_below"], frac["value_above"]) >= 0.10, (step, frac)


def test_adaptive_case_stays_clear_of_the_thresholds_and_moves_both_ways():
    case = ref.load_golden_case("mb3")
    assert case["ppo"]["schedule"] == "adaptive"
    _, _, _, trace, _ = _run(case, torch.float64)
    d = case["ppo"]["desired_kl"]
    for t in trace:
        for thr in (2.0 * d, d / 2.0):
            assert abs(t["kl"] - thr) >= 0.05 * thr, (t["kl"], thr)
    lrs = [case["ppo"]["learning_rate"]] + [t["learning_rate"] for t in trace]
    assert any(b > a for a, b in zip(lrs, lrs[1:])) and any(b < a for a, b in zip(lrs, lrs[1:])), lrs


def test_learning_rate_rule():
    assert ref.adaptive_learning_rate(1e-3, 0.03, 0.01) == 1e-3 / 1.5
    assert ref.adaptive_learning_rate(1e-3, 0.004, 0.01) == 1e-3 * 1.5
    assert ref.adaptive_learning_rate(1e-3, 0.01, 0.01) == 1e-3 and ref.adaptive_learning_rate(1e-3, 0.0, 0.01) == 1e-3
    assert ref.adaptive_learning_rate(1.2e-5, 1.0, 0.01) == 1e-5 and ref.adaptive_learning_rate(9e-3, 1e-4, 0.01) == 1e-2
