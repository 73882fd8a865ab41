"""The float64 restatement of `EmpiricalNormalization` (tests/normalizer_reference.py) against the reference module's own results
(tests/golden/empirical_normalization.npz, written by tools/refgen/make_runner_golden.py): every golden case, every call.  The module computes in
float32, so the bar is measured, not assumed: per case the largest deviation of the module's fp32 state and outputs from float64, in float32
ulp at the value's magnitude (`normalizer_reference.measure`), is computed from the fixture, printed, and held under `MODULE_BAR_ULP`.  That
bound is reasoning about the module's arithmetic: a float32 column mean / variance over n <= 1000 rows by torch's pairwise sums carries a few ulp
of the column's magnitude, the recurrences add a rounding per operation and per call (<= 6 calls), and a variance of data with mean 1e3 and spread 1e-2
is a difference of squares-sized quantities at 1e6 * 2^-24 -- which is why state and output carry separate figures and why the large-mean case alone
may reach the wider bound.  No GPU needed."""
import os

import numpy as np
import pytest

from tests import normalizer_reference as nr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "empirical_normalization.npz")
# fp32 against float64, in float32 ulp: sums of up to 1000 values, a handful of operations per call, six calls
MODULE_BAR_ULP = 64.0
# (mean 1e3, spread 1e-2, the batches 0.1 apart) in float32: from the second call on the module adds rate * delta * (mean_x - mean_new) to `_var`, where
# mean_x and mean_new are float32 values near 1e3, each off by up to half their spacing (6.1e-5), |delta| <= 0.3 and rate <= 1/2: up to
# 0.5 * 0.3 * 6.1e-5 = 9.2e-6 per call, 2.8e-5 over the three such calls, on a pooled variance of at least 0.05^2 = 2.5e-3 (two batches 0.1 apart):
# a relative 1.1e-2, which is 1.9e5 spacings of 2^-24 relative size
LARGE_MEAN_STATE_BAR_ULP = 1.9e5


@pytest.fixture(scope="module")
def golden():
    return nr.load_golden(GOLDEN)


def test_fixture_lists_the_cases_of_the_restatement(golden):
    z, cases = golden
    assert cases == nr.CASES
    names = [c["name"] for c in cases]
    assert [f"shape_{n}x{O}" for n, O in nr.SHAPES] == names[:6] and all(c["calls"] == 6 for c in cases[:6])
    assert {"constant_column", "large_mean_small_spread", "until_crossed", "eval_after_training", "inverse"} <= set(names)


@pytest.mark.parametrize("case", nr.CASES, ids=[c["name"] for c in nr.CASES])
def test_restatement_reproduces_the_module(golden, case):
    z, _ = golden
    name, batches = case["name"], nr.case_batches(case)
    for k, x in enumerate(batches[:case["calls"] + case["eval_calls"]]):
        assert x.dtype == np.float32 and x.shape == (case["n"], case["O"])
        assert float(x.astype(np.float64).sum()) == float(z[f"{name}.xsum{k}"]), "the regenerated batch is not the one the module saw"
    calls, inv = nr.run_case(case, batches)
    for k, c in enumerate(calls):
        assert int(z[f"{name}.count{k}"]) == c["count"], (name, k)
        assert z[f"{name}._mean{k}"].shape == (1, case["O"]) and z[f"{name}._mean{k}"].dtype == np.float32
    dev = nr.module_deviation(z, case, calls, inv, batches)
    print(f"{name}: module fp32 vs float64: state {dev['state']:.2f} ulp, output {dev['output']:.2f} ulp")
    assert np.isfinite(dev["state"]) and np.isfinite(dev["output"])
    assert dev["state"] <= (LARGE_MEAN_STATE_BAR_ULP if case["special"] == "large_mean" else MODULE_BAR_ULP), dev
    assert dev["output"] <= MODULE_BAR_ULP, dev


def test_special_cases_do_what_their_names_say(golden):
    z, _ = golden
    by = {c["name"]: c for c in nr.CASES}
    calls, _ = nr.run_case(by["until_crossed"])
    assert [c["count"] for c in calls] == [40, 80, 120, 120, 120]
    assert np.array_equal(calls[2]["mean"], calls[3]["mean"]) and np.array_equal(calls[3]["var"], calls[4]["var"])
    assert not np.array_equal(calls[1]["mean"], calls[2]["mean"])
    assert [int(z[f"until_crossed.count{k}"]) for k in range(5)] == [40, 80, 120, 120, 120]
    calls, _ = nr.run_case(by["eval_after_training"])
    assert [c["count"] for c in calls] == [50, 100, 150, 150, 150] and np.array_equal(calls[2]["std"], calls[4]["std"])
    calls, _ = nr.run_case(by["constant_column"])
    assert all(c["var"][2] == 0.0 and c["mean"][2] == 0.75 for c in calls) and all(np.all(c["y"][:, 2] == 0.0) for c in calls)
    calls, inv = nr.run_case(by["inverse"])
    m = nr.Float64Normalizer(11, 1e-3)
    m.mean, m.var, m.std = calls[-1]["mean"], calls[-1]["var"], calls[-1]["std"]
    np.testing.assert_allclose(m(inv, training=False), nr.case_batches(by["inverse"])[-1], rtol=1e-12, atol=1e-12)
