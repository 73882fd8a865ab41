"""Holds tests/ppo_recurrent_reference.py (the UNPADDED float64 / float32 torch restatement the GPU tests use) to tests/golden/ppo_update_recurrent.npz,
that is, to the reference's own padded `PPO.update` with `ActorCriticRecurrent` on torch-CPU: parameters, losses and the learning-rate trajectory
(exact), by the bar tests/test_ppo_update_reference.py uses for the feed-forward case.  This is the test that ties padded to unpadded.  Also, on the
restatement alone: the golden cases keep the float64 KL 5 % away from both thresholds, the episode-boundary rule is what the file says it is, and the
dones pattern covers what the GPU tests rely on.  No GPU needed."""
import pytest
import torch

from tests import ppo_recurrent_reference as rec
from tests import ppo_reference as ref


def _run(case, dtype):
    kw = case["ppo"]
    hyper = {k: kw[k] for k in ref.HYPER}
    return rec.update(case["sd0"], case["activation"], case["rnn_type"], case["rollout"], hyper, kw["num_learning_epochs"], kw["num_mini_batches"],
                      kw["learning_rate"], dtype)


@pytest.mark.parametrize("name", ["lstm", "gru"])
def test_unpadded_restatement_reproduces_the_references_padded_update(name):
    case = rec.load_golden_case(name)
    p32, loss32, lr32, trace32, _ = _run(case, torch.float32)
    p64, loss64, lr64, trace64, _ = _run(case, torch.float64)
    assert lr32 == case["learning_rate"] and lr64 == case["learning_rate"]
    assert [t["learning_rate"] for t in trace32] == case["lr_trajectory"] and [t["learning_rate"] for t in trace64] == case["lr_trajectory"]
    assert len(set(case["lr_trajectory"])) > 1          # desired_kl was chosen so that the learning rate moves
    for k, want in case["loss"].items():
        print(name, k, loss32[k], loss64[k], want)
        assert abs(loss32[k] - want) <= 2e-6 * abs(want), (k, loss32[k], want)
        assert abs(loss64[k] - want) <= 1e-5 * abs(want), (k, loss64[k], want)
    assert set(p64) == set(case["sd1"])
    for k, want in case["sd1"].items():
        scale = float(want.abs().max())
        moved = sum(case["lr_trajectory"])          # see tests/test_ppo_update_reference.py: an Adam step moves a parameter by about lr
        assert float((p32[k] - want).abs().max()) <= 0.02 * moved + 1e-6 * scale, k
        assert float((p64[k].float() - want).abs().max()) <= 0.10 * moved + 1e-6 * scale, k
        assert float((p64[k].float() - want).abs().mean()) <= 1e-5 * max(scale, 1.0), k


@pytest.mark.parametrize("name", ["lstm", "gru"])
def test_golden_rollout_stays_clear_of_the_thresholds_and_has_the_dones_pattern(name):
    case = rec.load_golden_case(name)
    _, _, _, trace, _ = _run(case, torch.float64)
    kw, ro = case["ppo"], case["rollout"]
    for t in trace:
        for thr in (2.0 * kw["desired_kl"], kw["desired_kl"] / 2.0):
            assert abs(t["kl"] - thr) >= 0.05 * thr, (t["kl"], thr)
    d = ro["dones"]
    assert d.shape == (8, 12) and {(t, e) for t, e in d.nonzero().tolist() if e != 6} == {(0, 1), (7, 2), (3, 3), (4, 3), (6, 4), (2, 5), (5, 5), (1, 9)}
    assert bool(d[:, 6].all()) and float(ro["h_a"][0].abs().max()) > 0          # one env done at every step; the state at t = 0 is not zero


@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_episode_boundaries_of_the_restatement(rnn_type):
    sd = rec.random_params(rnn_type, 2, 8, 5, 6, [7], [7], 3, seed=1)
    ro = rec.craft_rollout(sd, "elu", rnn_type, 5, 12, seed=2)
    mu0, v0, _, _ = rec.forward(sd, "elu", rnn_type, ro, 0, 12)
    mu0, v0 = mu0.view(5, 12, -1), v0.view(5, 12, -1)
    d = ro["dones"]
    t, e = 1, 3          # dones_pattern(5, 12): env 3 is done at steps 1 and 2
    assert d[t, e] == 1 and d[t + 1, e] == 1
    other = dict(ro, observations=ro["observations"].clone())
    other["observations"][:t + 1, e] += 1.0          # before the done: nothing after it moves
    mu1 = rec.forward(sd, "elu", rnn_type, other, 0, 12)[0].view(5, 12, -1)
    assert torch.equal(mu1[t + 1:, e], mu0[t + 1:, e]) and not torch.equal(mu1[:t + 1, e], mu0[:t + 1, e])
    other = dict(ro, h_a=ro["h_a"].clone())
    other["h_a"][t + 1, :, e] += 0.5          # the saved row at a trajectory start is what the step enters with
    mu2 = rec.forward(sd, "elu", rnn_type, other, 0, 12)[0].view(5, 12, -1)
    assert not torch.equal(mu2[t + 1, e], mu0[t + 1, e]) and torch.equal(mu2[:t + 1], mu0[:t + 1])
    other = dict(ro, h_a=ro["h_a"].clone())
    other["h_a"][1, :, 0] += 0.5          # env 0 is never done: its saved row at t = 1 is not a start and is never read
    assert d[:, 0].sum() == 0
    assert torch.equal(rec.forward(sd, "elu", rnn_type, other, 0, 12)[0], mu0.view(60, -1))


@pytest.mark.parametrize("T,N", [(5, 37), (7, 75), (3, 33), (1, 37), (8, 12)])
def test_dones_pattern_covers_the_cases(T, N):
    d = rec.dones_pattern(T, N)
    assert d.shape == (T, N) and bool(d[:, 6].all()) and int((d.sum(0) == 0).sum()) >= 3          # one env done at every step, several never
    if T > 1:
        assert d[0].sum() >= 1 and d[T - 1].sum() >= 2          # a done at t = 0 and at t = T - 1 (beside the always-done env)
    if T >= 5:
        assert bool(((d[:-1] * d[1:]).sum(0) > 0)[[e for e in range(N) if e % 12 != 6]].any())          # consecutive steps
