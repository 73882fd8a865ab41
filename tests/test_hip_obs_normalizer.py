"""`lg_obsnorm` (include/lgrunner.h, csrc/lg_runner.hip) through `rl.NativeEmpiricalNormalization` on every golden case of
tests/golden/empirical_normalization.npz: the state after each call and the outputs against the float64 restatement
(tests/normalizer_reference.py).  Per case the bar is twice the reference module's own fp32 deviation from float64 on that case, taken from the
fixture at test time, never below 4 ulp at the value's magnitude (`normalizer_reference.measure` says what that magnitude is).

Measured on MI355X (float32 ulp; native / module / bar = max(2 x module, 4)), state then output:
    shape_1x1 0.90 / 1.84 / 4.00, 0.33 / 0.33 / 4.00;  shape_3x7 5.33 / 20.33 / 40.67, 1.11 / 1.16 / 4.00;  shape_64x48 2.06 / 9.00 / 17.99, 2.85 / 2.80 / 5.60
    shape_65x235 11.36 / 22.63 / 45.25, 3.59 / 7.57 / 15.13;  shape_257x253 5.36 / 23.08 / 46.17, 5.61 / 3.79 / 7.58
    shape_1000x260 12.37 / 26.36 / 52.73, 7.19 / 6.54 / 13.07;  constant_column 0.65 / 0.65 / 4.00, 1.69 / 2.07 / 4.14
    large_mean_small_spread 3143 / 36320 / 72640, 1.73 / 2.60 / 5.20;  until_crossed 0.88 / 1.19 / 4.00, 2.00 / 2.76 / 5.53
    eval_after_training 2.15 / 12.22 / 24.44, 1.85 / 1.85 / 4.00;  inverse 3.00 / 7.34 / 14.69, 2.44 / 7.23 / 14.45
The state figures are what keeping `_mean` / `_var` in float32 between calls costs (the restatement keeps float64); DESIGN.md section 11g.
"""
import os

import numpy as np
import pytest
import torch

from tests import normalizer_reference as nr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "empirical_normalization.npz")
IDS = [c["name"] for c in nr.CASES]


def make(case):
    from extended_legged_gym_amd.rl import NativeEmpiricalNormalization
    return NativeEmpiricalNormalization([case["O"]], eps=case["eps"], until=case["until"], device="cuda:0")


def run_native(case, batches, mode="out"):
    """Per call (mean, var, std, count, y) of the native normaliser.  mode: out (a fresh output), inplace, strided (rows of a wider buffer)."""
    m = make(case)
    got = []
    for k in range(case["calls"] + case["eval_calls"]):
        m.train(k < case["calls"])
        x = torch.from_numpy(batches[k]).cuda()
        if mode == "inplace":
            y = m.normalize_(x.clone())
        elif mode == "strided":
            wide = torch.full((case["n"], case["O"] + 5), float("nan"), device="cuda")
            wide[:, :case["O"]] = x
            y = m(wide[:, :case["O"]])
            assert y.shape == x.shape
        else:
            y = m(x)
        mean, var, std, count = m.get_state()
        got.append(dict(_mean=mean, _var=var, _std=std, count=count, y=y.cpu().numpy()))
    inv = m.inverse(torch.from_numpy(batches[-1]).cuda()).cpu().numpy() if case["special"] == "inverse" else None
    return got, inv, m


@pytest.fixture(scope="module")
def golden():
    return nr.load_golden(GOLDEN)


@pytest.mark.parametrize("case", nr.CASES, ids=IDS)
def test_state_and_outputs_against_float64_within_twice_the_modules_own_deviation(golden, case):
    z, _ = golden
    batches = nr.case_batches(case)
    calls, inv = nr.run_case(case, batches)
    bars = nr.bars(nr.module_deviation(z, case, calls, inv, batches))
    got, got_inv, _ = run_native(case, batches)
    for k, c in enumerate(calls):
        assert got[k]["count"] == c["count"] == int(z[f"{case['name']}.count{k}"]), k
    dev = nr.measure(case, calls, inv, batches, lambda kind, k: got_inv if k is None else got[k][kind])
    print(f"{case['name']}: native state {dev['state']:.2f} ulp (bar {bars['state']:.2f}), output {dev['output']:.2f} ulp (bar {bars['output']:.2f})")
    assert dev["state"] <= bars["state"] and dev["output"] <= bars["output"], (dev, bars)


@pytest.mark.parametrize("case", nr.CASES, ids=IDS)
def test_two_runs_in_place_and_strided_rows_give_the_same_bits(case):
    batches = nr.case_batches(case)
    a, a_inv, _ = run_native(case, batches)
    for mode in ("out", "inplace", "strided"):
        b, b_inv, _ = run_native(case, batches, mode)
        for k in range(len(a)):
            for key in ("_mean", "_var", "_std", "y"):
                assert np.array_equal(a[k][key], b[k][key]), (mode, k, key)
            assert a[k]["count"] == b[k]["count"]
        assert a_inv is None or np.array_equal(a_inv, b_inv)


def test_update_zero_leaves_the_state_untouched_and_update_alone_writes_nothing():
    case = nr.CASES[3]
    batches = nr.case_batches(case)
    m = make(case)
    m(torch.from_numpy(batches[0]).cuda())
    before = m.get_state()
    m.eval()
    y = m(torch.from_numpy(batches[1]).cuda())
    after = m.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3] == after[3] == case["n"]
    want = (batches[1] - before[0]) / (before[2] + np.float32(case["eps"]))
    assert np.array_equal(y.cpu().numpy(), want.astype(np.float32))          # the module's two float32 operations
    m.update(torch.from_numpy(batches[1]).cuda())          # update() counts whatever the mode
    assert m.get_state()[3] == 2 * case["n"] and int(m.count) == 2 * case["n"]
    assert torch.equal(m.mean.cpu(), torch.from_numpy(m.get_state()[0])) and m.std.shape == (case["O"],)


def test_until_freezes_the_state_and_the_count():
    case = next(c for c in nr.CASES if c["name"] == "until_crossed")
    got, _, m = run_native(case, nr.case_batches(case))
    assert [g["count"] for g in got] == [40, 80, 120, 120, 120]
    for key in ("_mean", "_var", "_std"):
        assert np.array_equal(got[2][key], got[3][key]) and np.array_equal(got[3][key], got[4][key]) and not np.array_equal(got[1][key], got[2][key])


def test_state_round_trip_is_exact_and_state_dict_is_the_modules():
    case = nr.CASES[2]
    got, _, m = run_native(case, nr.case_batches(case))
    state = m.get_state()
    other = make(case)
    other.set_state(*state)
    back = other.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(state[:3], back[:3])) and state[3] == back[3]
    sd = m.state_dict()
    assert list(sd) == ["_mean", "_var", "_std", "count"] and sd["_mean"].shape == (1, case["O"]) and sd["count"].dtype == torch.long
    third = make(case)
    third.load_state_dict(sd)
    x = torch.from_numpy(nr.case_batches(case)[0]).cuda()
    assert torch.equal(third.eval()(x), m.eval()(x))
    # the state the module itself reached loads too, and normalises as the module did
    z, _ = nr.load_golden(GOLDEN)
    k, name = case["calls"] - 1, case["name"]
    third.load_state_dict({"_mean": torch.from_numpy(z[f"{name}._mean{k}"]), "_var": torch.from_numpy(z[f"{name}._var{k}"]),
                           "_std": torch.from_numpy(z[f"{name}._std{k}"]), "count": torch.tensor(int(z[f"{name}.count{k}"]))})
    y = third(torch.from_numpy(nr.case_batches(case)[k]).cuda()).cpu().numpy()
    assert np.array_equal(y[nr.kept_rows(case)], z[f"{name}.y{k}"])


def test_no_rows_is_a_no_op_and_bad_rows_are_refused():
    case = nr.CASES[1]
    m = make(case)
    before = m.get_state()
    y = m(torch.empty(0, case["O"], device="cuda"))
    assert y.shape == (0, case["O"]) and m.get_state()[3] == 0 and all(np.array_equal(a, b) for a, b in zip(before[:3], m.get_state()[:3]))
    with pytest.raises(ValueError):
        m(torch.zeros(4, case["O"] + 1, device="cuda"))
    assert m.carried_row(4) is None
    # in place means in place: inputs the kernels would have to convert first are refused, not normalised as a copy
    for bad in (torch.zeros(4, case["O"]), torch.zeros(4, case["O"], device="cuda", dtype=torch.float64), torch.zeros(case["O"], 4, device="cuda").t()):
        with pytest.raises(ValueError, match="in place"):
            m.normalize_(bad)
    x = torch.ones(4, case["O"], device="cuda")
    assert m.normalize_(x) is x and m.count.device.type == "cuda" and int(m.count) == 4
