"""GPU: `NativeRecurrentPPO` on memories with more than 512 inputs (`lg_rnn_create_wide` handles in `lg_ppo_recurrent_create`): the forward with saved
gates is one projection launch over the mini-batch + the seeded tile per step, the backward is the narrow trainer's, `weight_ih_l0` is a segment of
the slab weight-gradient pass over the gathered observation rows.

Against tests/ppo_recurrent_reference.py in float64, at the bar of tests/test_hip_ppo_recurrent_update.py (taken from that file): e <= max(8 e32, 2e-5),
e32 the restatement in fp32 against itself in float64 on the same inputs; both printed before they are asserted.  Sizes: T = 6, 24 envs, episodes
that end inside the window, hidden 40, heads [32, 16]; the actor's memory on 578 columns and the critic's on 1041 (W1, LSTM), the reverse with a
narrow critic (W2, GRU: a mixed pair), and two layers (W3).
Exact: the training forward equals the rows the act produced during collection; two updates from one state give equal bits; a policy rebuilt from
`state_dict()` acts with the bits of the one the trainer moved; `optimizer_state()` into a new trainer continues with equal bits."""
import pytest
import torch

from tests import ppo_recurrent_reference as rec
from tests import ppo_reference as ref
from tests.test_hip_ppo_recurrent_update import ACT, DEV, _build, _native, _state_equal
from tests.test_hip_ppo_update import _err, _within

pytestmark = pytest.mark.gpu
T, N = 6, 24
SHAPES = {          # rnn_type, layers, obs, critic obs, std key
    "W1": ("lstm", 1, 578, 1041, "std"),
    "W2": ("gru", 1, 1041, 48, "log_std"),
    "W3": ("gru", 2, 578, 578, "std"),
}
_CACHE = {}


def _case(shape):
    """(state dict, rollout on the CPU, rnn_type, std type): built once per shape and left unchanged."""
    if shape not in _CACHE:
        rnn_type, L, O, Oc, std_key = SHAPES[shape]
        sd = rec.random_params(rnn_type, L, 40, O, Oc, [32, 16], [32, 16], 12, seed=51, std_key=std_key)
        ro = rec.craft_rollout(sd, ACT, rnn_type, T, N, seed=52)
        assert 0 < float(ro["dones"][:-1].sum()) < (T - 1) * N          # episodes end inside the window
        _CACHE[shape] = (sd, ro, rnn_type, "scalar" if std_key == "std" else "log")
    return _CACHE[shape]


@pytest.mark.parametrize("shape,clipped", [("W1", True), ("W1", False), ("W2", True), ("W3", True)])
def test_gradients_losses_and_norm_against_float64(shape, clipped):
    sd, ro, rnn_type, std_type = _case(shape)
    hyper = dict(ref.HYPER, use_clipped_value_loss=clipped, entropy_coef=0.01, value_loss_coef=0.8)
    policy, ppo = _build(sd, rnn_type, std_type, **hyper)
    ppo.minibatch(_native(ro), 0, N)
    g, norm, means = ppo.gradients()
    g64, n64, m64, _, _, _, _ = rec.gradients(sd, ACT, rnn_type, ro, 0, N, hyper, torch.float64)
    g32, n32, m32, _, _, _, _ = rec.gradients(sd, ACT, rnn_type, ro, 0, N, hyper, torch.float32)
    assert set(g) == set(g64) and g["memory_a.rnn.weight_ih_l0"].shape[1] == SHAPES[shape][2] and g["memory_c.rnn.weight_ih_l0"].shape[1] == SHAPES[shape][3]
    ok = True
    for k in g64:
        ok &= _within(f"{shape} {k}", _err(g[k], g64[k]), _err(g32[k], g64[k]))
    ok &= _within(f"{shape} norm", abs(norm - float(n64)) / float(n64), abs(float(n32) - float(n64)) / float(n64))
    for k in ("surrogate", "value_function", "entropy", "kl"):
        ok &= _within(f"{shape} {k}", abs(means[k] - float(m64[k])) / abs(float(m64[k])), abs(float(m32[k]) - float(m64[k])) / abs(float(m64[k])))
    assert ok
    for k in ("memory_a", "memory_c"):          # every column of the wide rows reaches its weight, past the last slab edge too
        w = g[f"{k}.rnn.weight_ih_l0"]
        assert float(w[:, -1].abs().max()) > 0.0 and (w.shape[1] <= 512 or float(w[:, 512].abs().max()) > 0.0)


@pytest.mark.parametrize("rnn_type", ["lstm", "gru"])
def test_training_forward_equals_the_collected_rows_and_the_weights_move(rnn_type):
    """A rollout collected by the recurrent act on 578-wide rows: the trainer's forward gives its `mu` and `values` bit for bit; one update moves the
    weights, the policy acts with them, and a policy rebuilt from `state_dict()` gives the same bits."""
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent
    O, H, M = 578, 40, 2
    sd = rec.random_params(rnn_type, 1, H, O, O, [32, 16], [32, 16], 12, seed=61)
    policy, ppo = _build(sd, rnn_type, "scalar", learning_rate=3e-3, num_mini_batches=M, num_learning_epochs=2, **ref.HYPER)
    g = torch.Generator().manual_seed(62)
    obs = torch.randn(T, N, O, generator=g).to(DEV)
    dones = (torch.rand(T, N, generator=g) < 0.2).float().to(DEV)
    policy.act_and_evaluate(obs[0])          # one step lived: the first saved state is not zero

    def flat(hs):
        return list(hs) if isinstance(hs, tuple) else [hs]
    rows = {k: [] for k in ("actions", "values", "actions_log_prob", "mu", "sigma")}
    hid = {"a": [], "c": []}
    for t in range(T):
        ha, hc = policy.get_hidden_states()
        hid["a"].append([h.clone() for h in flat(ha)]); hid["c"].append([h.clone() for h in flat(hc)])
        a, v, lp, mu, sig = policy.act_and_evaluate(obs[t])
        for k, x in zip(rows, (a, v, lp.view(-1, 1), mu, sig)):
            rows[k].append(x.clone())
        policy.reset(dones[t])
    out = {k: torch.stack(v) for k, v in rows.items()}
    out.update(observations=obs, dones=dones.unsqueeze(-1), returns=out["values"] + 0.3 * torch.randn(T, N, 1, generator=g).to(DEV),
               advantages=torch.randn(T, N, 1, generator=g).to(DEV))
    for tag in ("a", "c"):
        stacks = tuple(torch.stack([step[j] for step in hid[tag]]) for j in range(len(hid[tag][0])))
        out["hidden_states_" + tag] = stacks if rnn_type == "lstm" else stacks[0]
    mb = N // M
    ppo.minibatch(out, 0, mb)
    mu, val = ppo.forward_outputs(T * mb)          # unchanged parameters: the collected rows, bit for bit
    assert torch.equal(mu.view(T, mb, -1), out["mu"][:, :mb].cpu()) and torch.equal(val.view(T, mb, 1), out["values"][:, :mb].cpu())
    ppo.update(out)
    new_sd = ppo.state_dict()
    assert set(new_sd) == set(sd) and all(not torch.equal(new_sd[k], sd[k]) for k in sd if "weight" in k)
    fresh = NativeActorCriticRecurrent(new_sd, ACT, rnn_type, device=DEV, seed=1)
    older = NativeActorCriticRecurrent(sd, ACT, rnn_type, device=DEV, seed=1)
    for p in (policy, fresh, older):
        p.reset()
    a, b, c = policy.act_inference(obs[0]), fresh.act_inference(obs[0]), older.act_inference(obs[0])
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(policy.evaluate(obs[0]), fresh.evaluate(obs[0]))


def test_updates_are_deterministic_and_the_optimiser_state_round_trips():
    sd, ro, rnn_type, std_type = _case("W1")
    kw = dict(ref.HYPER, schedule="adaptive", desired_kl=0.004, entropy_coef=0.005, learning_rate=4e-3, num_learning_epochs=2, num_mini_batches=2)
    rows = _native(ro)
    _, one = _build(sd, rnn_type, std_type, **kw)
    _, two = _build(sd, rnn_type, std_type, **kw)
    loss1, loss2 = one.update(rows), two.update(rows)
    s1 = one.optimizer_state()
    assert loss1 == loss2 and s1["step"] == 4
    _state_equal(s1, two.optimizer_state())
    # optimizer_state() -> a new trainer -> load_optimizer_state(): the next update is the first trainer's
    _, three = _build(sd, rnn_type, std_type, **kw)
    three.load_optimizer_state(s1)
    _state_equal(s1, three.optimizer_state())
    loss1b, loss3 = one.update(rows), three.update(rows)
    assert loss1b == loss3
    _state_equal(one.optimizer_state(), three.optimizer_state())
    print("workspace bytes at", T * N // 2, "rows:", one.workspace_bytes() if hasattr(one, "workspace_bytes") else "n/a")


def test_the_other_trainers_refuse_a_wide_memory_by_name(monkeypatch):
    """`lg_distill_rtrain_create`, `lg_estimator_train_create` and `lg_estimator_step` name the wide memory they are given; nothing is launched and the
    refused handles still act."""
    from extended_legged_gym_amd import abi
    from extended_legged_gym_amd.rl import NativeEstimatorDistillation, NativeRecurrentDistillation, NativeStudentTeacherRecurrent, NativeTerrainEstimator
    from tests import estimator_update_reference as eref
    torch.manual_seed(71)
    rnn = torch.nn.LSTM(578, 40, 1)

    def seq(i):
        return torch.nn.Sequential(torch.nn.Linear(i, 32), torch.nn.ELU(), torch.nn.Linear(32, 12))
    sd = {"std": torch.ones(12)}
    for prefix, module in (("student", seq(40)), ("teacher", seq(48)), ("memory_s.rnn", rnn)):
        sd.update({f"{prefix}.{k}": v.detach().clone() for k, v in module.state_dict().items()})
    policy = NativeStudentTeacherRecurrent(sd, activation="elu", rnn_type="lstm", device=DEV, seed=3)
    assert policy.memory_s.input_size == 578
    alg = NativeRecurrentDistillation(policy, sd)
    with pytest.raises(RuntimeError, match=r"lg_distill_rtrain_create: the memory is a wide one \(lg_rnn_create_wide, 578 inputs\)"):
        alg._create(64)
    obs, tobs = torch.randn(9, 578).to(DEV), torch.randn(9, 48).to(DEV)
    actions, teacher_actions = policy.act_and_teach(obs, tobs)
    assert bool(torch.isfinite(actions).all()) and float(policy.memory_s.h.abs().max()) > 0.0
    # the estimator's memory reads the combination layer (<= 512 columns): only the diagnostic switch makes it a wide one
    case = eref.group_cases()[0]
    state = case.state()
    monkeypatch.setenv("LG_RNN_FORCE_WIDE", "1")
    monkeypatch.setattr(abi, "RNN_MAX_WIDTH", 0)          # NativeMemory then takes lg_rnn_create_wide whatever the width
    est = NativeTerrainEstimator(state, case.shape, case.P, activation=case.act, memory_type=case.memory, device=DEV)
    monkeypatch.undo()
    depth, prop = torch.rand(5, *case.shape).to(DEV), torch.randn(5, case.P).to(DEV)
    with pytest.raises(RuntimeError, match=r"lg_estimator_step: the memory is a wide one \(lg_rnn_create_wide"):
        est.act_inference(depth, prop)
    trainer = NativeEstimatorDistillation(est, state, gradient_length=case.G, loss_type=case.loss)
    with pytest.raises(RuntimeError, match=r"lg_estimator_train_create: the memory is a wide one \(lg_rnn_create_wide"):
        trainer._create(64)
    top = est.memory(torch.randn(5, est.memory.input_size).to(DEV))
    assert bool(torch.isfinite(top).all()) and float(top.abs().max()) > 0.0
